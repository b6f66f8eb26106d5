"""-m gpu: action-prefix conditioning of the flow head (fv_head_set_flow_prefix) -- the noising kernel's PREFIX instance (explicit and drawn delays), one head
step against float64 autograd, the S-draw identity, the prefix sampler against its float64 reference, its bit rules, the older entry points on a
prefix-width head, the off switch, and the toy the feature exists for.

Bars.  Prepare: torch.equal against the plain flow handle (the same kernel body) and against targets.  Head step: test_gpu_flow's, loss 1e-5 relative,
velocity rtol 1e-4 / atol 1e-5, gradients 2e-5 max(1e-3, max |ref|).  S-draw identity: test_gpu_flow_draws' three-way comparison.  Sampler: worst row
against the RMS row norm, at most 4 x the distance of the fp32 CPU emulation from float64 on the same case (tests/test_flow_prefix_host.py keeps that
distance below 1e-4 for every case used here)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_draws_util as du  # noqa: E402
import flow_prefix_util as pu  # noqa: E402
import flow_util as fu  # noqa: E402
import rtc_util as ru  # noqa: E402
from chunk_loss_util import ragged_pad  # noqa: E402
from gpu_util import DEV  # noqa: E402
from fastvla_hip import HEAD_KEYS, FastVLAEngine, _lib, arch, prefix  # noqa: E402
from fastvla_hip.engine import flow_draw_offset  # noqa: E402
from fastvla_hip.rtc import prefix_weights  # noqa: E402


PINNED_REFERENCE = 1.0      # the torch reference's pinned fraction on the toy (tests/test_flow_prefix_host.py asserts it reaches this)


def _engine(name, B, D=None, S=1, dims=None, max_batch=None, dist="uniform", rate=0.0):
    """a head-only engine in flow mode; D: prefix mode with that largest delay (None: the plain flow head)"""
    feat, ds, hid, fus, K, A, E = dims or fu.DIMS[name]
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=ds, action_dim=K * A, hidden_dim=hid, fusion_dim=fus, max_batch=max_batch or max(B, 1))
    eng.set_head_flow(E)
    if D is not None:
        eng.set_head_flow_prefix(K, D, dist=dist, rate=rate)
    if S > 1:
        eng.set_head_flow_draws(S)
    return eng


def _flat(eng, p):
    flat = torch.zeros(eng.head_numel(), device=DEV)
    for k, v in eng.head_views(flat).items():
        v.copy_(p[k])
    return flat


def _set_io(eng, st, on):
    if on:
        eng.set_io_norm(st["state_mean"], st["state_std"], st["action_mean"], st["action_std"])
    else:
        eng.set_io_norm()


def _up4(n):
    return (n + 3) // 4 * 4


def _grad_bar(r):
    return 2e-5 * max(1e-3, float(r.abs().max()))


def _mixed_delays(R, D):
    """0, 1 and D mixed across the rows, one above D (clamped) once there are four rows"""
    d = np.array([(D, 0, 1, D + 3)[r % 4] for r in range(R)], dtype=np.int32)
    return d


# ------------------------------------------------------------------------------------------------------------------ 1. prepare, explicit noise, t and delays
@pytest.mark.parametrize("B", [1, 9, 67])
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_prepare_with_explicit_noise_t_and_delays(name, B):
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da, D, xo = K * A, pu.MAX_DELAY[name], feat + hid
    eng, plain = _engine(name, B, D), _engine(name, B)
    g = torch.Generator().manual_seed(5 + B)
    a, eps, t = torch.randn(B, da, generator=g), torch.randn(B, da, generator=g), torch.rand(B, generator=g)
    delays = _mixed_delays(B, D)
    saved, saved_p = eng.head_saved(B).fill_(float("nan")), plain.head_saved(B).fill_(float("nan"))
    u = eng.head_flow_prepare(a, saved, noise=eps, t=t, delays=torch.from_numpy(delays))
    u_p = plain.head_flow_prepare(a, saved_p, noise=eps, t=t)
    torch.cuda.synchronize()
    cat, cat_p = pu.saved_cat(eng, saved, B), pu.saved_cat(plain, saved_p, B)
    pin = np.minimum(delays, D)                                      # a delay above D is clamped
    pinned = torch.from_numpy(pu.mask_ref(pin, K)).bool().repeat_interleave(A, dim=1).to(DEV)
    x, x_p = cat[:, xo:xo + da], cat_p[:, xo:xo + da]
    assert torch.equal(x[pinned], a.to(DEV)[pinned])                 # the prefix is a copy of the targets
    assert torch.equal(x[~pinned], x_p[~pinned])                     # everything else is the plain head's
    assert torch.equal(cat[:, xo + da:xo + da + E], cat_p[:, xo + da:]) and torch.equal(u, u_p)
    m = cat[:, xo + da + E:]
    assert m.shape == (B, K) and torch.equal(m, torch.from_numpy(pu.mask_ref(pin, K)).float().to(DEV))
    # the byte mask sits behind everything else in `saved`; nothing but cat's three column blocks and it was written
    nb = _up4((B * K + 3) // 4)                                      # (every block inside `saved` is rounded up to 16 bytes)
    got_bytes = saved[-nb:].view(torch.uint8)[:B * K].view(B, K)
    assert torch.equal(got_bytes.cpu(), torch.from_numpy(pu.mask_ref(pin, K)).to(torch.uint8))
    rest = torch.ones_like(saved, dtype=torch.bool)
    rest[-nb:] = False
    off = cat.storage_offset() - saved.storage_offset()
    rest[off:off + B * cat.shape[1]].view(B, -1)[:, xo:] = False
    assert bool(torch.isnan(saved[rest]).all())
    eng.close(), plain.close()


# ------------------------------------------------------------------------------------------------------------------ 2. drawn delays
@pytest.mark.parametrize("name,dist,rate", [("awkward", "uniform", 0.0), ("larger", "exp", 0.3)])
def test_drawn_delays_match_the_philox_reference(name, dist, rate):
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da, D, xo, B, seed, offset = K * A, pu.MAX_DELAY[name], feat + hid, 67, 0x1234_5678_9ABC, 77
    eng, plain = _engine(name, B, D, dist=dist, rate=rate), _engine(name, B)
    thr = prefix.delay_thresholds(D, dist, rate)

    def run(e, Bc, off_):
        saved = e.head_saved(Bc)
        u = e.head_flow_prepare(torch.zeros(Bc, da), saved, seed=seed, offset=off_)
        torch.cuda.synchronize()
        return pu.saved_cat(e, saved, Bc).clone().cpu(), u.cpu()

    for off_ in (offset, offset + 1):
        cat, u = run(eng, B, off_)
        cat_p, u_p = run(plain, B, off_)
        got = cat[:, xo + da + E:].sum(dim=1).to(torch.int64).numpy()
        want = pu.draw_delays(B, seed, off_, thr)
        assert np.array_equal(got, want), (got, want)
        assert torch.equal(cat[:, xo + da + E:], torch.from_numpy(pu.mask_ref(want, K)).float())
        # t and eps are the plain handle's draws: u = eps (a = 0) everywhere, phi(t) bit for bit, x_t = t eps outside the prefix
        assert torch.equal(u, u_p) and torch.equal(cat[:, xo + da:xo + da + E], cat_p[:, xo + da:])
        free = ~torch.from_numpy(pu.mask_ref(want, K)).bool().repeat_interleave(A, dim=1)
        assert torch.equal(cat[:, xo:xo + da][free], cat_p[:, xo:xo + da][free])
    assert len(set(pu.draw_delays(B, seed, offset, thr).tolist())) > 1
    cat3, _ = run(eng, 3, offset)                                    # row b's delay does not depend on B
    assert np.array_equal(cat3[:, xo + da + E:].sum(dim=1).to(torch.int64).numpy(), pu.draw_delays(B, seed, offset, thr)[:3])
    eng.close(), plain.close()


# ------------------------------------------------------------------------------------------------------------------ 3. one head step against float64 autograd
def _weights(A, K, seed):
    g = torch.Generator().manual_seed(seed)
    dim_w, step_w = torch.rand(A, generator=g) * 2.0 + 0.25, torch.rand(K, generator=g) * 2.0 + 0.25
    dim_w[A - 1] = 0.0
    return dim_w, step_w


def _step(eng, flat, c, delays, pad, B, **draw):
    saved = eng.head_saved(B)
    if delays is None:
        u = eng.head_flow_prepare(c["a"][:B], saved, **draw)
    else:
        u = eng.head_flow_prepare(c["a"][:B], saved, noise=c["eps"][:B], t=c["t"][:B], delays=torch.from_numpy(np.asarray(delays[:B])))
    v, _ = eng.head_forward(flat, c["pooled"][:B].to(DEV), c["states"][:B].to(DEV), saved=saved, normalized_actions=True)
    loss, grads = eng.head_backward(flat, v, u, saved, pad=pad)
    torch.cuda.synchronize()
    return loss.clone(), grads.clone(), v.clone(), u.clone(), saved


def _prefix_step_case(name, B, seed=0):
    c = dict(du.case(name, B, 1, seed=seed))
    K = c["dims"][4]
    g = torch.Generator().manual_seed(31 + B)
    w = c["p"]["fusion.0.weight"]
    c["p"] = dict(c["p"])
    c["p"]["fusion.0.weight"] = torch.cat([w, torch.randn(w.shape[0], K, generator=g) * float(w.std())], dim=1)
    return c


@pytest.mark.parametrize("kind,padded,weighted", [("mse", False, False), ("mse", True, False), ("l1", True, False), ("l1", False, True), ("mse", True, True)])
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_prefix_head_step_matches_float64_autograd(name, B, kind, padded, weighted):
    c = _prefix_step_case(name, B)
    feat, ds, hid, fus, K, A, E = c["dims"]
    D = pu.MAX_DELAY[name]
    pad = ragged_pad(B, K, seed=1) if padded else None
    w = _weights(A, K, 3) if weighted else None
    delays = _mixed_delays(B, D)
    eng = _engine(name, B, D)
    eng.set_head_loss(kind, 1.0, K)
    if w is not None:
        eng.set_head_loss_weights(*w)
    flat = _flat(eng, c["p"])
    loss, grads, v, u, _ = _step(eng, flat, c, delays, pad, B)
    ref = pu.step_reference(c["p"], c["pooled"], c["states"], c["a"], c["eps"], c["t"], np.minimum(delays, D), pad, kind, c["dims"], *(w or (None, None)))
    np.testing.assert_allclose(v.cpu().numpy(), ref["pred"].numpy(), rtol=1e-4, atol=1e-5)
    rl = float(ref["loss"])
    el = abs(float(loss) - rl) / rl if rl > 0 else abs(float(loss))
    gv = eng.head_views(grads)
    worst = max(float((gv[k].cpu().double() - ref["grads"][k]).abs().max()) / _grad_bar(ref["grads"][k]) for k in HEAD_KEYS)
    print(f"[prefix head step {name} B={B} {kind} pad={padded} weighted={weighted}] loss rel {el:.2e}; worst gradient error / bar {worst:.3f}")
    assert el <= 1e-5
    for k in HEAD_KEYS:
        err = float((gv[k].cpu().double() - ref["grads"][k]).abs().max())
        assert err <= _grad_bar(ref["grads"][k]), (k, err, _grad_bar(ref["grads"][k]))
    # the valid fraction stays the pad-only one; the masked MSE runs over the trained elements
    met = eng.head_loss_metrics().cpu().double()
    padt = torch.from_numpy(pad if pad is not None else np.zeros((B, K), dtype=bool))
    assert abs(float(met[1]) - float((~padt).double().mean())) <= 1e-6
    if not weighted:
        d = (v.cpu().double() - u.cpu().double()).view(B, K, A)
        live = (~(padt | torch.from_numpy(pu.mask_ref(np.minimum(delays, D), K)).bool())).unsqueeze(-1).expand_as(d)
        mse = float((d * d)[live].sum() / d.numel())
        assert abs(float(met[0]) - mse) <= 1e-5 * max(1e-3, mse)
    eng.close()


@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_a_fully_masked_row_contributes_nothing(name, kind):
    """row 8 has delay D and every later step padded: the 9-row batch's sums (loss and gradients times their element count) are the 8-row batch's"""
    B = 9
    c = _prefix_step_case(name, B)
    feat, ds, hid, fus, K, A, E = c["dims"]
    D, da = pu.MAX_DELAY[name], K * A
    delays = _mixed_delays(B, D)
    delays[B - 1] = D
    pad = ragged_pad(B, K, seed=1)
    pad[B - 1] = False
    pad[B - 1, D:] = True
    out = {}
    for Bc in (B, B - 1):
        eng = _engine(name, Bc, D)
        eng.set_head_loss(kind, 1.0, K)
        flat = _flat(eng, c["p"])
        loss, grads, _, _, _ = _step(eng, flat, c, delays, pad[:Bc], Bc)
        out[Bc] = (float(loss) * Bc * da, {k: g.cpu().double() * Bc * da for k, g in eng.head_views(grads).items()})
        eng.close()
    ref = pu.step_reference(c["p"], c["pooled"][:B - 1], c["states"][:B - 1], c["a"][:B - 1], c["eps"][:B - 1], c["t"][:B - 1], np.minimum(delays[:B - 1], D),
                            pad[:B - 1], kind, c["dims"])
    n = (B - 1) * da
    assert abs(out[B][0] - out[B - 1][0]) <= 1e-5 * float(ref["loss"]) * n
    for k in HEAD_KEYS:
        assert float((out[B][1][k] - out[B - 1][1][k]).abs().max()) <= _grad_bar(ref["grads"][k]) * n, k


@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_zero_delays_are_the_plain_flow_head(name):
    B = 9
    c = _prefix_step_case(name, B)
    feat, ds, hid, fus, K, A, E = c["dims"]
    D = pu.MAX_DELAY[name]
    eng, plain = _engine(name, B, D), _engine(name, B)
    for e in (eng, plain):
        e.set_head_loss("mse", 1.0, K)
    loss, grads, v, _, _ = _step(eng, _flat(eng, c["p"]), c, np.zeros(B, dtype=np.int32), None, B)
    cp = dict(c)
    cp["p"] = pu.drop_mask_columns(c["p"], K)
    sv = plain.head_saved(B)
    u = plain.head_flow_prepare(c["a"], sv, noise=c["eps"], t=c["t"])
    flat_p = _flat(plain, cp["p"])
    vp, _ = plain.head_forward(flat_p, c["pooled"].to(DEV), c["states"].to(DEV), saved=sv, normalized_actions=True)
    loss_p, grads_p = plain.head_backward(flat_p, vp, u, sv)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_p)) <= 1e-6 * float(loss_p)
    gv, gp = eng.head_views(grads), plain.head_views(grads_p)
    for k in HEAD_KEYS:
        a_, b_ = gv[k].cpu().double(), gp[k].cpu().double()
        if k == "fusion.0.weight":
            assert bool((a_[:, -K:] == 0).all())                    # the mask columns saw m = 0: their gradient is exactly 0
            a_ = a_[:, :-K]
        assert float((a_ - b_).abs().max()) <= 1e-6 * float(b_.abs().max()), k
    eng.close(), plain.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the S-draw identity
@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("name,B", [("awkward", 9), ("larger", 1)])
def test_s_draw_prefix_step_is_the_mean_of_s_single_draw_steps(name, B, kind):
    """test_gpu_flow_draws' identity with the delays drawn too: draw s of the S-draw step at offset o is the single draw at o + (s << 56), delay included"""
    S = 3
    c = _prefix_step_case(name, B, seed=1)
    feat, ds, hid, fus, K, A, E = c["dims"]
    da, D, seed, o, xo = K * A, pu.MAX_DELAY[name], 991, du.train_offset(3, 1000, 1), feat + hid
    pad = ragged_pad(B, K, seed=2) if B > 1 else None
    eng, one = _engine(name, B, D, S=S), _engine(name, B, D)
    for e in (eng, one):
        e.set_head_loss(kind, 1.0, K)
    flat = _flat(eng, c["p"])
    # what the device drew, read back exactly: targets 0 gives u = eps, noise 1 gives x_t = t outside the prefix (the last step is never conditioned on)
    saved = eng.head_saved(B)
    eps = eng.head_flow_prepare(torch.zeros(B, da), saved, seed=seed, offset=o).cpu()
    eng.head_flow_prepare(torch.zeros(B, da), saved, seed=seed, offset=o, noise=torch.ones(S * B, da))
    torch.cuda.synchronize()
    cat = pu.saved_cat(eng, saved, B)
    t, delays = cat[:, xo + da - 1].clone().cpu(), cat[:, xo + da + E:].sum(dim=1).to(torch.int64).cpu().numpy()
    thr = prefix.delay_thresholds(D)
    assert np.array_equal(delays, np.concatenate([pu.draw_delays(B, seed, flow_draw_offset(o, s), thr) for s in range(S)]))

    lm, gm, vm, _, _ = _step(eng, flat, c, None, pad, B, seed=seed, offset=o)
    singles = [_step(one, flat, c, None, pad, B, seed=seed, offset=flow_draw_offset(o, s)) for s in range(S)]
    assert all(torch.equal(vm[s * B:(s + 1) * B], singles[s][2]) for s in range(S))
    lm, ls = float(lm), sum(float(x[0]) for x in singles) / S
    gs = sum(x[1].double() for x in singles) / S
    each = [pu.step_reference(c["p"], c["pooled"], c["states"], c["a"], eps[s * B:(s + 1) * B], t[s * B:(s + 1) * B], delays[s * B:(s + 1) * B], pad, kind, c["dims"])
            for s in range(S)]
    rl = float(sum(r["loss"] for r in each) / S)
    assert abs(lm - rl) <= 1e-5 * rl and abs(ls - rl) <= 1e-5 * rl and abs(lm - ls) <= 2e-5 * rl
    vm_, vs_ = eng.head_views(gm), eng.head_views(gs)
    worst = 0.0
    for k in HEAD_KEYS:
        r = sum(x["grads"][k] for x in each) / S
        bar_m, bar_s = _grad_bar(r), sum(_grad_bar(x["grads"][k]) for x in each) / S
        em, es = float((vm_[k].cpu().double() - r).abs().max()), float((vs_[k].cpu() - r).abs().max())
        eb = float((vm_[k].cpu().double() - vs_[k].cpu()).abs().max())
        worst = max(worst, em / bar_m, es / bar_s, eb / (bar_m + bar_s))
        assert em <= bar_m and es <= bar_s and eb <= bar_m + bar_s, (k, em, bar_m, es, bar_s, eb)
    print(f"[prefix draws identity {name} B={B} {kind}] loss S-draw {lm:.6f} mean of singles {ls:.6f} float64 {rl:.6f}; worst error / bar {worst:.3f}")
    eng.close(), one.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the sampler against prefix_euler_sample
@pytest.mark.parametrize("B", fu.SAMPLER_BATCHES)
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_prefix_sampler_matches_float64_reference(name, B):
    c = pu.prefix_case(name, B)
    K = c["dims"][4]
    eng = _engine(name, B, c["D"])
    flat = _flat(eng, c["p"])
    pooled, states, prev, delays = c["pooled"].to(DEV), c["states"].to(DEV), c["prev"].to(DEV), torch.from_numpy(c["delays"]).to(DEV)
    worst = 0.0
    for shift in pu.SHIFTS(K):
        for io in (False, True):
            _set_io(eng, c["stats"], io)
            for N in fu.SAMPLER_STEPS:
                act, chunk = eng.head_flow_sample_prefix(flat, pooled, states, prev, delays, shift=shift, steps=N, noise=c["noise"])
                torch.cuda.synchronize()
                a64, c64, ea, ec = pu.prefix_refs(name, B, N, io, shift)
                for what, got, ref, emu in (("actions", act, a64, ea), ("chunk_out", chunk, c64, ec)):
                    err = fu.worst_row_vs_rms(got.cpu(), ref)
                    worst = max(worst, err / (4 * emu))
                    print(f"[prefix sampler {name} B={B} shift={shift} N={N} io={int(io)}] {what}: error {err:.3e}, fp32 emulation {emu:.3e}, "
                          f"error / bar {err / (4 * emu):.3f}")
                    assert bool(torch.isfinite(got).all()) and err <= 4 * emu
    print(f"[prefix sampler {name} B={B}] worst error / bar {worst:.3f}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6. bit rules
@pytest.mark.parametrize("name,B", [("awkward", 9), ("larger", 67), ("larger", 1)])
def test_prefix_sampler_bit_rules(name, B):
    c = pu.prefix_case(name, B)
    K, A, D = c["dims"][4], c["dims"][5], c["D"]
    da, N, st = K * A, 4, c["stats"]
    eng = _engine(name, B, D)
    flat = _flat(eng, c["p"])
    pooled, states, prev = c["pooled"].to(DEV), c["states"].to(DEV), c["prev"].to(DEV)
    delays = torch.from_numpy(c["delays"]).to(DEV)
    _set_io(eng, st, True)
    std, mean = st["action_std"].to(DEV), st["action_mean"].to(DEV)

    def run(prev_, delays_, shift):
        a_, c_ = eng.head_flow_sample_prefix(flat, pooled, states, prev_, delays_, shift=shift, steps=N, noise=c["noise"])
        torch.cuda.synchronize()
        return a_.clone(), c_.clone()

    zero = run(prev, torch.zeros_like(delays), 0)
    for shift in pu.SHIFTS(K) + (K,):
        act, chunk = run(prev, delays, shift)
        again = run(prev, delays, shift)
        assert torch.equal(act, again[0]) and torch.equal(chunk, again[1])                         # two calls agree
        pin = pu.pinned_steps(c["delays"], D, K, shift)
        assert shift < K or int(pin.max()) == 0                                                    # shift = K pins nothing
        poisoned, poisoned_rows = prev.clone(), prev.clone()
        for b in range(B):
            n = int(pin[b]) * A
            want = prev[b, shift * A:shift * A + n]
            assert torch.equal(chunk[b, :n], want)                                                 # the pinned elements are prev's bits
            assert torch.equal(act[b, :n], torch.addcmul(mean[:n].double(), want.double(), std[:n].double()).float())      # fmaf(prev, std, mean): one rounding
            if pin[b] == 0:
                assert torch.equal(act[b], zero[0][b]) and torch.equal(chunk[b], zero[1][b])       # a row with delay 0 is the all-zero-delay call's row
                poisoned[b] = float("nan")
            else:
                poisoned[b, :shift * A] = float("inf")
                poisoned[b, shift * A + n:] = float("nan")
        pa, pc = run(poisoned, delays, shift)
        assert torch.equal(pa, act) and torch.equal(pc, chunk)                                     # NaN / inf outside the pinned ranges changes no bit
        if int(pin.max()) > 0:
            b = int(np.argmax(pin))
            poisoned_rows[b, shift * A] = float("nan")                                             # NaN inside a pinned range stays in its own row
            na, nc = run(poisoned_rows, delays, shift)
            others = [r for r in range(B) if r != b]
            assert bool(torch.isnan(nc[b]).any())
            assert torch.equal(na[others], act[others]) and torch.equal(nc[others], chunk[others])
    # no delays pin nothing and add no mask column: the plain sampler's bits on the same handle, whatever the shift (one step: the first stage is the final one)
    none = torch.zeros_like(delays)
    for io in (False, True):
        _set_io(eng, st, io)
        for steps in (1, 4):
            plain = eng.head_flow_sample(flat, pooled, states, steps=steps, noise=c["noise"]).clone()
            for shift in (0, 2, K):
                a_, c_ = eng.head_flow_sample_prefix(flat, pooled, states, prev, none, shift=shift, steps=steps, noise=c["noise"])
                torch.cuda.synchronize()
                assert torch.equal(a_, plain) and (io or torch.equal(c_, plain)), (io, steps, shift)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 7. the older entry points on a prefix-width head
def test_plain_and_guided_samplers_on_a_prefix_width_head():
    name, B, N = "larger", 9, 10
    c = pu.prefix_case(name, B)
    K, A, E, D = c["dims"][4], c["dims"][5], c["dims"][6], c["D"]
    d, s, shift = ru.rtc_config(K, "third")
    w = prefix_weights(K, d, s, "exp")
    eng = _engine(name, B, D)
    eng.set_head_flow_guidance(w, ru.BETA)
    flat = _flat(eng, c["p"])
    pooled, states = c["pooled"].to(DEV), c["states"].to(DEV)
    plain_p = pu.drop_mask_columns(c["p"], K)                         # with m = 0 the head is the plain one without the mask columns
    got = eng.head_flow_sample(flat, pooled, states, steps=N, noise=c["noise"])
    act, chunk = eng.head_flow_sample_guided(flat, pooled, states, c["prev"].to(DEV), shift=shift, steps=N, noise=c["noise"])
    torch.cuda.synchronize()
    ref = fu.euler_sample(plain_p, c["pooled"], c["states"], c["noise"], N, E)
    emu = fu.worst_row_vs_rms(fu.euler_sample_fp32(plain_p, c["pooled"], c["states"], c["noise"], N, E), ref)
    err = fu.worst_row_vs_rms(got.cpu(), ref)
    print(f"[prefix-width head, plain sampler] error {err:.3e}, bar {4 * emu:.3e}")
    assert err <= 4 * emu
    Y, W = ru.targets(c["prev"], ru.prefix_weights_ref(K, d, s, "exp"), K, A, shift)
    args = (plain_p, c["pooled"], c["states"], c["noise"], N, E, Y, W, ru.BETA)
    a64, c64 = ru.guided_euler(*args)
    a32, c32 = ru.guided_euler(*args, fp32=True)
    for what, g_, r_, e_ in (("actions", act, a64, a32), ("chunk_out", chunk, c64, c32)):
        err, emu = fu.worst_row_vs_rms(g_.cpu(), r_), fu.worst_row_vs_rms(e_, r_)
        print(f"[prefix-width head, guided sampler] {what}: error {err:.3e}, bar {4 * emu:.3e}")
        assert err <= 4 * emu
    # fv_head_forward at inference zeroes the mask columns: the velocity at (x, t) is the plain head's
    saved = eng.head_saved(B)
    pu.saved_cat(eng, saved, B)[:, -K:] = 1.0
    x, t = c["noise"], torch.full((B,), 0.5)
    eng.head_flow_prepare(x, saved, noise=x, t=t, delays=torch.full((B,), D, dtype=torch.int32))
    v, _ = eng.head_forward(flat, pooled, states, saved=saved)
    torch.cuda.synchronize()
    assert bool((pu.saved_cat(eng, saved, B)[:, -K:] == 0).all())
    v64 = fu.velocity({k: q.double() for k, q in plain_p.items()}, c["pooled"].double(), c["states"].double(), x.double(),
                      torch.from_numpy(fu.phi_ref(t.numpy(), fu.flow_freqs(E))))
    np.testing.assert_allclose(v.cpu().numpy(), v64.numpy(), rtol=1e-4, atol=1e-5)
    eng.close()


def test_vjp_op_on_a_prefix_width_head():
    """fv_op_flow_vjp_prefix: the guided step's chain on the wide row stride against float64 autograd with the mask columns dropped (m = 0), at
    test_gpu_rtc's bar for the same op: 4 x the fp32 emulation's distance"""
    from gpu_util import lib, stream
    name, B = "larger", 9
    c = pu.prefix_case(name, B)
    feat, ds, hid, fus, K, A, E = c["dims"]
    da = K * A
    eng = _engine(name, B, c["D"])
    flat = _flat(eng, c["p"])
    plain_p = pu.drop_mask_columns(c["p"], K)
    freq = torch.from_numpy(fu.flow_freqs(E)).to(DEV)
    pooled, states, xd = c["pooled"].to(DEV), c["states"].to(DEV), c["noise"].to(DEV)
    om = torch.randn(B, da, generator=torch.Generator().manual_seed(90 + B))
    omd, scr = om.to(DEV), torch.zeros(1 << 21, device=DEV)
    for t in (1.0, 0.5):
        v, jt = torch.full((B, da), float("nan"), device=DEV), torch.full((B, da), float("nan"), device=DEV)
        _lib.check(lib().fv_op_flow_vjp_prefix(feat, ds, da, hid, fus, E, K, freq.data_ptr(), flat.data_ptr(), pooled.data_ptr(), states.data_ptr(), B, xd.data_ptr(), t,
                                               omd.data_ptr(), v.data_ptr(), jt.data_ptr(), scr.data_ptr(), scr.numel(), stream()), "fv_op_flow_vjp_prefix")
        torch.cuda.synchronize()
        v64, jt64 = ru.vjp_ref(plain_p, c["pooled"], c["states"], c["noise"], t, om, E)
        v32, jt32 = ru.vjp_ref(plain_p, c["pooled"], c["states"], c["noise"], t, om, E, fp32=True)
        for what, got, ref, emu in (("v", v, v64, v32), ("J^T omega", jt, jt64, jt32)):
            bar, err = 4 * fu.worst_row_vs_rms(emu, ref), fu.worst_row_vs_rms(got.cpu(), ref)
            print(f"[prefix-width vjp t={t:.2f}] {what}: error {err:.3e}, bar {bar:.3e}")
            assert bool(torch.isfinite(got).all()) and err <= bar
    bad = lambda k_, n_: lib().fv_op_flow_vjp_prefix(feat, ds, da, hid, fus, E, k_, freq.data_ptr(), flat.data_ptr(), pooled.data_ptr(), states.data_ptr(), B,  # noqa: E731
                                                     xd.data_ptr(), 1.0, omd.data_ptr(), v.data_ptr(), jt.data_ptr(), scr.data_ptr(), n_, stream())
    assert bad(K, 16) == -1 and bad(1, scr.numel()) == -1 and bad(da + 1, scr.numel()) == -1
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 8. off means off
def test_off_means_off_and_the_setter_checks():
    name, B = "awkward", 5
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da, D = K * A, pu.MAX_DELAY[name]
    fresh, seen = _engine(name, B), _engine(name, B)
    L = seen.lib
    thr = (C.c_uint32 * (D + 1))(*prefix.delay_thresholds(D))

    def sizes(e):
        n, wsb, offs = C.c_size_t(), C.c_size_t(), (C.c_int64 * 13)()
        assert L.fv_head_saved_bytes(e.h, B, C.byref(n)) == 0 and L.fv_head_layout(e.h, C.byref(offs)) == 0
        assert L.fv_workspace_bytes(e.h, B, 1, 0, C.byref(wsb)) == 0
        return n.value, wsb.value, list(offs)

    base = sizes(fresh)
    # the existing formulas: fusion.0 has feat + hid + da + E columns
    assert base[2][5] - base[2][4] == (fus * (feat + hid + da + E) + 3) // 4 * 4
    bad = [(K, 0), (K, K), (K, -1), (1, 1), (2, 1), (da + 1, 1)]       # D outside 1 .. K - 1, K < 2, K that does not divide action_dim
    for k_, d_ in bad:
        assert L.fv_head_set_flow_prefix(seen.h, k_, d_, thr) == -1, (k_, d_)
    for table in ([5, 4, 1 << 24], [1, 2, 3], [0, (1 << 24) + 1, 1 << 24]):   # not monotone, not ending at 2^24, above 2^24
        assert L.fv_head_set_flow_prefix(seen.h, K, D, (C.c_uint32 * 3)(*table)) == -1, table
    assert L.fv_head_set_flow_prefix(None, K, D, thr) == -1
    assert sizes(seen) == base
    # prefix entry points with the mode off: FV_ERR_STATE
    buf = torch.full((4096,), float("nan"), device=DEV)
    iz = torch.zeros(B, dtype=torch.int32, device=DEV)
    p_ = buf.data_ptr()
    assert L.fv_head_flow_prepare_prefix(seen.h, p_, 1, 0, 0, None, None, iz.data_ptr(), p_, p_, None) == -2
    assert L.fv_head_flow_sample_prefix(seen.h, p_, p_, p_, 1, 10, None, 0, 0, p_, 0, iz.data_ptr(), p_, None, None) == -2
    # on: the sizes grow by the K mask columns (and the byte mask inside saved); NULL returns to the plain flow head's
    seen.set_head_flow_prefix(K, D)
    on = sizes(seen)
    assert on[2][5] - on[2][4] == (fus * (feat + hid + da + E + K) + 3) // 4 * 4 and on[1] >= base[1]
    cw = feat + hid + da + E
    assert on[0] == base[0] + 4 * (_up4(B * (cw + K)) - _up4(B * cw) + _up4((B * K + 3) // 4))
    assert seen.head_cat_width() == feat + hid + da + E + K
    seen.set_head_flow_prefix(None)
    assert sizes(seen) == base and seen.head_offsets == fresh.head_offsets
    seen.set_head_flow_prefix(K, D)
    seen.set_head_flow(None)                                           # fv_head_set_flow(NULL) switches it off too
    seen.set_head_flow(E)
    assert sizes(seen) == base
    # argument checks of the sampler, nothing enqueued
    seen.set_head_flow_prefix(K, D)
    flat = torch.zeros(seen.head_numel(), device=DEV)
    pooled, states = torch.zeros(B, feat, device=DEV), torch.zeros(B, ds, device=DEV)
    out, prev = torch.full((B, da), float("nan"), device=DEV), torch.zeros(B, da, device=DEV)
    args = (flat.data_ptr(), pooled.data_ptr(), states.data_ptr())
    call = lambda B_, n_, shift_, prev_=prev.data_ptr(), dl_=iz.data_ptr(), fp_=args[0]: L.fv_head_flow_sample_prefix(  # noqa: E731
        seen.h, fp_, args[1], args[2], B_, n_, None, 0, 0, prev_, shift_, dl_, out.data_ptr(), None, None)
    assert call(B, 10, 0) == -2                                        # no workspace bound yet
    seen.ensure_workspace(B, 1, False)
    assert call(B, 0, 0) == -1 and call(B, 10, -1) == -1 and call(B, 10, K + 1) == -1 and call(B + 1, 10, 0) == -1 and call(0, 10, 0) == -1
    assert call(B, 10, 0, prev_=None) == -1 and call(B, 10, 0, dl_=None) == -1 and call(B, 10, 0, fp_=None) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the workspace is bound: sizes depend on the mode, so the setter refuses both ways and changes nothing
    before = sizes(seen)
    assert L.fv_head_set_flow_prefix(seen.h, 0, 0, None) == -2 and L.fv_head_set_flow_prefix(seen.h, K, 1, (C.c_uint32 * 2)(1 << 23, 1 << 24)) == -2
    assert b"fv_bind_workspace" in L.fv_last_error(seen.h) and sizes(seen) == before
    assert call(B, 10, K) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    # a flow handle that never called the setter computes a step's bits as a handle that switched the mode on and off again
    toggled = _engine(name, B)
    toggled.set_head_flow_prefix(K, D)
    toggled.set_head_flow_prefix(None)
    c = du.case(name, B, 1)
    outs = []
    for e in (fresh, toggled):
        e.set_head_loss("l1", 1.0, K)
        fl = _flat(e, c["p"])
        sv = e.head_saved(B)
        u = e.head_flow_prepare(c["a"], sv, seed=3, offset=9)
        v, _ = e.head_forward(fl, c["pooled"].to(DEV), c["states"].to(DEV), saved=sv, normalized_actions=True)
        loss, grads = e.head_backward(fl, v, u, sv, pad=ragged_pad(B, K, seed=1))
        smp = e.head_flow_sample(fl, c["pooled"].to(DEV), c["states"].to(DEV), steps=4, seed=1, offset=2)
        torch.cuda.synchronize()
        outs.append((v.clone(), loss.clone(), grads.clone(), smp.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    fresh.close(), seen.close(), toggled.close()


# ------------------------------------------------------------------------------------------------------------------ 9. the property the feature exists for
def test_bimodal_toy_a_pinned_first_step_selects_the_mode():
    """flow_prefix_util.PREFIX_BIMODAL on the project's kernels and AdamW: every target chunk lies wholly in the + or wholly in the - mode.  Pinning the first
    step to a + chunk's puts the other three steps in the + mode; without a pin both modes appear.  The torch reference of the same recipe
    (tests/test_flow_prefix_host.py) reaches a pinned fraction of 1.000; the bar here is that minus 0.05, a 4 sigma binomial margin at n = 512 near 0.9."""
    r = pu.PREFIX_BIMODAL
    feat, ds, hid, fus, K, A, E = r["dims"]
    da, B, D, n = K * A, r["batch"], r["D"], r["samples"]
    eng = _engine(None, B, D, dims=r["dims"], max_batch=n)
    eng.set_head_loss("mse", 1.0, K)
    flat = _flat(eng, pu.prefix_bimodal_init(r["seed"]))
    targets = fu.bimodal_targets(B, da, r["seed"]).to(DEV)
    pooled, states = fu.bimodal_observation(B, feat, ds)
    pooled, states = pooled.to(DEV), states.to(DEV)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    saved = eng.head_saved(B)
    for it in range(1, r["steps"] + 1):
        u = eng.head_flow_prepare(targets, saved, seed=11, offset=it)
        out, _ = eng.head_forward(flat, pooled, states, saved=saved, normalized_actions=True)
        _, grads = eng.head_backward(flat, out, u, saved)
        eng.adamw_step(flat, grads, m, v, it, lr=r["lr"], weight_decay=0.0, max_grad_norm=0.0)
    po, so = pooled[:1].expand(n, -1).contiguous(), states[:1].expand(n, -1).contiguous()
    prev = torch.ones(n, da, device=DEV)
    _, pinned = eng.head_flow_sample_prefix(flat, po, so, prev, torch.ones(n, dtype=torch.int32), steps=10, seed=5, offset=1)
    _, free = eng.head_flow_sample_prefix(flat, po, so, prev, torch.zeros(n, dtype=torch.int32), steps=10, seed=5, offset=2)
    torch.cuda.synchronize()
    ps, fs = pu.pinned_stats(pinned.cpu()), fu.mode_stats(free.cpu())
    print(f"[prefix bimodal] pinned: {ps}; free: {fs}")
    assert torch.equal(pinned[:, :A], prev[:, :A])
    assert ps["plus"] >= PINNED_REFERENCE - 0.05
    assert fs["plus"] >= 0.25 and fs["minus"] >= 0.25 and fs["mean_abs"] >= 0.7
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 10. surfaces
ENV_KEYS = ("FASTVLA_RTC", "FASTVLA_RTC_METHOD", "FASTVLA_RTC_PREFIX_STEPS", "FASTVLA_ACTION_HEAD", "FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "FASTVLA_FLOW_PREFIX_MAX_DELAY",
            "FASTVLA_FLOW_PREFIX_DELAY_DIST", "FASTVLA_FLOW_PREFIX_DELAY_RATE", "FASTVLA_FLOW_NOISE_DRAWS", "FASTVLA_FLOW_STEPS", "FASTVLA_EMA_DECAY",
            "FASTVLA_LORA_RANK", "FASTVLA_TRAIN_TOWER")
PK, PN, PD = 8, 3, 3      # chunk, n_action_steps, largest delay of the policy-level tests


def _policy(prefix_delay=PD, seed=0, **kw):
    from vla_fastvlm.fastvla.configuration_fastvla import FastVLAConfig
    from vla_fastvlm.fastvla.modeling_fastvla import FastVLAPolicy
    torch.manual_seed(seed)
    extra = {} if prefix_delay is None else {"flow_prefix_max_delay": prefix_delay}
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=PK, n_action_steps=PN,
                         action_head="flow", flow_time_dim=6, flow_seed=77, **extra, **kw).to(DEV)


def test_backbone_routes_inherit_the_prefix_loss():
    """the "small" model's full, projected-LoRA and direct-LoRA train steps in prefix mode (the routes noise their targets through the shared prepare and take
    the shared head backward) against the head-only route on the same (seed, offset): test_gpu_flow_draws' comparison and bars for the same pair"""
    from oracle import fastvit_hd
    from fastvla_hip import weights
    from gpu_util import rel_l2
    r, GRAD_TOL = pu.ROUTE, pu.ROUTE_GRAD_TOL
    model = arch.preset("small")
    B, T, K, da, hd, E, D = r["B"], r["T"], r["K"], r["K"] * r["A"], r["hd"], r["E"], 2
    w = weights.init_backbone(model, seed=41)
    eng = FastVLAEngine(model, state_dim=14, action_dim=da, hidden_dim=hd, fusion_dim=hd, max_batch=B, max_text_tokens=T, llm_precision=1)
    eng.set_head_flow(E)
    eng.set_head_flow_prefix(K, D)                                    # (where it has to be: before train_begin)
    eng.load_weights(w)
    eng.train_begin()
    _, total, _ = eng.train_layout()
    flat = torch.zeros(total, dtype=torch.float32, device=DEV)
    eng.train_export_params(flat)
    g = torch.Generator().manual_seed(42)
    shapes = pu.prefix_head_shapes(model.llm.hidden, 14, da, hd, hd, E, K)
    hp = {k: (torch.randn(*s_, generator=g) / (s_[-1] ** 0.5 if len(s_) > 1 else 10.0)) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
          for k, s_ in shapes.items()}
    for k, v in eng.head_views(flat).items():
        v.copy_(hp[k])
    tower_out, ids, mask, states = pu.route_inputs(model, B, T, 42)
    targets = torch.randn(B, da, generator=torch.Generator().manual_seed(43))
    eng.set_head_loss("mse", 1.0, K)
    ws = eng.train_workspace(B, T)
    scale = eng.train_loss_scale()
    common = (tower_out.to(DEV), ids, mask.sum(1), states, targets, ws)
    off_ = r["offset"]
    assert int(pu.draw_delays(B, r["seed"], off_, prefix.delay_thresholds(D)).max()) > 0          # some step of this batch is conditioned on

    def head_only():
        with torch.no_grad():
            tok = fastvit_hd.projector_forward(w, tower_out.float()).to(DEV)
        pooled = eng.llm_pooled(ids, mask.sum(1), tok)
        hflat = flat[: eng.head_numel()].clone()
        saved = eng.head_saved(B)
        u = eng.head_flow_prepare(targets, saved, seed=r["seed"], offset=off_)
        v, _ = eng.head_forward(hflat, pooled, states.to(DEV), saved=saved, normalized_actions=True)
        loss, grads = eng.head_backward(hflat, v, u, saved)
        torch.cuda.synchronize()
        return v.clone(), float(loss), grads.clone()

    out = {"head_full": head_only()}
    a, l, g_ = eng.train_forward_backward(flat, *common, training=False, seed=r["seed"], offset=off_, flat_grads=torch.zeros_like(flat))
    torch.cuda.synchronize()
    out["full"] = (a.clone(), float(l), g_ / scale)
    eng.train_lora_begin(r["rank"], 2.0 * r["rank"], None)
    lt, ltotal = eng.train_lora_layout()
    lflat = torch.zeros(ltotal, device=DEV)
    front = lt[16]["offset"]
    lflat[:front].copy_(flat[:front])
    pu.random_adapters(lflat, lt, seed=9)
    eng.train_lora_commit(flat, lflat)
    out["head_lora"] = head_only()
    a, l, g_ = eng.train_forward_backward(flat, *common, training=False, seed=r["seed"], offset=off_, flat_grads=torch.zeros_like(flat))
    lg = torch.zeros_like(lflat)
    eng.train_lora_project(g_, lflat, lg)
    torch.cuda.synchronize()
    out["proj"] = (a.clone(), float(l), lg / scale)
    a, l, g_ = eng.train_lora_forward_backward(flat, lflat, *common, training=False, seed=r["seed"], offset=off_, lora_grads=torch.zeros_like(lflat))
    torch.cuda.synchronize()
    out["direct"] = (a.clone(), float(l), g_ / scale)
    hn = eng.head_numel()
    views = lambda t: {k: x.clone() for k, x in eng.head_views(t[:hn]).items()}  # noqa: E731
    for route, ref in (("full", "head_full"), ("proj", "head_lora")):
        v, loss, gr = out[route]
        rv, rl, rg = out[ref]
        got, want = views(gr), views(rg)
        errs = sorted(((rel_l2(got[k].cpu(), want[k].cpu()), k) for k in HEAD_KEYS), reverse=True)
        ra, el = rel_l2(v.cpu(), rv.cpu()), abs(loss - rl) / rl
        print(f"[prefix route {route} vs head-only] velocity rel_l2 {ra:.2e} loss rel {el:.2e}; worst head gradients: " + "; ".join(f"{k} {e:.2e}" for e, k in errs[:3]))
        assert ra <= 1e-3 and el <= 1e-3 and all(e <= GRAD_TOL for e, _ in errs), errs[:3]
    assert torch.equal(out["direct"][0], out["proj"][0]) and out["direct"][1] == out["proj"][1] and torch.equal(out["direct"][2][:hn], out["proj"][2][:hn])
    eng.close()


@pytest.mark.parametrize("route", ["head", "draws"])      # (the routes that exist for the tiny model: its decoder's head_dim rules out backbone training)
def test_prefix_policy_trains_two_steps_on_every_route(route, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    B = 4
    pol = _policy(flow_noise_draws=3) if route == "draws" else _policy()
    pol.train()
    losses = []
    for s in (41, 42):
        out = pol.fused_train_step(pu.policy_batch(B, PK, s, DEV), lr=1e-3)
        losses.append(float(out["loss"]))
        assert out["actions"].shape == (B, PK, 14)
    torch.cuda.synchronize()
    eng = pol.model._engine()
    assert eng.head_flow_prefix["max_delay"] == PD and eng.head_cat_width() == pol.model.fusion[0].in_features
    assert all(np.isfinite(x) and x > 0 for x in losses) and bool(torch.isfinite(pol.model._flat).all())
    # the chunked loss ran (plain MSE included) and reports the pad-only valid fraction: row 0 of the batch has its last step padded
    met = eng.head_loss_metrics().cpu()
    assert abs(float(met[1]) - (1.0 - 1.0 / (B * PK))) <= 1e-6
    # compute_loss in train() mode trains the head; in eval() mode the loss, delays included, depends on the evaluation batch index only
    batch = pu.policy_batch(B, PK, 5, DEV)
    res = pol.compute_loss(batch)
    res["loss"].backward()
    assert all(p_.grad is not None and bool(torch.isfinite(p_.grad).all()) for p_ in pol.model.head_parameters())
    pol.eval()
    with torch.no_grad():
        e1 = [float(pol.compute_loss(b)["loss"]) for b in (batch, batch)]
    pol.eval()
    with torch.no_grad():
        e2 = [float(pol.compute_loss(b)["loss"]) for b in (batch, batch)]
    assert e1 == e2 and e1[0] != e1[1]
    eng.close()


def test_core_policy_replans_with_a_pinned_prefix(tmp_path, monkeypatch):
    import json
    from vla_fastvlm.training import Trainer, TrainingConfig
    from vla_fastvlm.utils import load_policy_from_checkpoint
    from vla_fastvlm.utils.checkpoint import save_policy_checkpoint
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    K, n, D, A = PK, PN, PD, 14
    pol, plain = _policy(rtc=True, rtc_method="prefix"), _policy()
    assert pol.rtc == {"method": "prefix", "prefix_steps": D, "max_delay": D} and plain.rtc is None
    pol.train()
    for s in (41, 42):                                            # a trained head: the mask columns are in use
        pol.fused_train_step(pu.policy_batch(4, K, s, DEV), lr=1e-3)
    plain.load_state_dict(pol.state_dict())
    g = torch.Generator().manual_seed(5)
    img, st, task = torch.rand(3, 72, 96, generator=g).to(DEV), torch.randn(14, generator=g).to(DEV), "open drawer"
    served, plans = [], []
    for i in range(3 * n + 1):                                    # three re-plans behind the first plan
        prev = pol.last_chunk_normalised
        served.append(pol.select_action(img, st, task, DEV))
        if i % n == 0:
            plans.append((prev, pol.last_chunk_normalised))
    assert pol.model._flow_sample_calls == 4 and pol.model._engine().head_flow_guidance is None
    first = [plain.select_action(img, st, task, DEV) for _ in range(n)]
    assert all(torch.equal(a, b) for a, b in zip(served[:n], first))                             # the first plan pins nothing: the policy without rtc
    pins = min(D, K - n)
    for j, (prev, chunk) in enumerate(plans):
        assert all(torch.equal(served[j * n + r], chunk[r]) for r in range(min(n, len(served) - j * n)))
        if j:
            assert torch.equal(chunk[:pins], prev[n:n + pins]) and not torch.equal(chunk[pins], prev[n + pins])      # the steps being executed are the old plan's, exactly
    # reset(): the next plan asks for D pinned steps like every plan (select_action passes no delay) and pins nothing, because reset() cleared the row's
    # previous chunk -- the policy without rtc serves the same bits.  Counter-check: the same call WITHOUT reset() does pin.
    before = pol.last_chunk_normalised
    calls = pol.model._flow_sample_calls
    pinned_plan = pol.select_action_chunk(img, st, task, DEV)                                     # no reset, no explicit delay: rtc_prefix_steps = D steps
    assert torch.equal(pinned_plan[:D], before[:D]) and not torch.equal(pinned_plan[D], before[D])
    plain.model._flow_sample_calls = calls
    assert not torch.equal(pinned_plan, plain.select_action_chunk(img, st, task, DEV))
    pol.reset(), plain.reset()
    plain.model._flow_sample_calls = pol.model._flow_sample_calls
    after = [pol.select_action(img, st, task, DEV) for _ in range(n)]
    assert all(torch.equal(a, b) for a, b in zip(after, [plain.select_action(img, st, task, DEV) for _ in range(n)]))
    assert not torch.equal(pol.last_chunk_normalised[:D], pinned_plan[:D])
    pol.reset(), plain.reset()
    plain.model._flow_sample_calls = pol.model._flow_sample_calls
    assert torch.equal(pol.select_action_chunk(img, st, task, DEV), plain.select_action_chunk(img, st, task, DEV))      # the explicit form after reset(): likewise
    last = pol.last_chunk_normalised
    got = pol.select_action_chunk(img, st, task, DEV, prev_chunk=last[n:], inference_delay=2)
    assert torch.equal(got[:2], last[n:n + 2]) and not torch.equal(got[2], last[n + 2]) and torch.equal(pol.last_chunk_normalised, got)
    with pytest.raises(ValueError, match="inference_delay=4"):
        pol.select_action_chunk(img, st, task, DEV, prev_chunk=last[n:], inference_delay=D + 1)
    # save and reload: the record, and the reloaded policy samples the same bits
    ck = save_policy_checkpoint(pol, tmp_path / "prefix")
    rec = json.loads((ck / "hip_extras.json").read_text())["action_head"]
    assert rec["prefix_max_delay"] == D and rec["prefix_delay_dist"] == "uniform"
    back = load_policy_from_checkpoint(str(ck), DEV).to(DEV)
    assert back.flow_prefix == pol.flow_prefix and back.rtc is None                               # rtc is a property of the run
    plain.model._flow_sample_calls = back.model._flow_sample_calls
    assert torch.equal(back.select_action_chunk(img, st, task, DEV), plain.select_action_chunk(img, st, task, DEV))
    # a plain flow checkpoint fails to load into a prefix policy, naming the two shapes; widened, it loads and samples the plain policy's chunk
    flow = _policy(prefix_delay=None, seed=3)
    flow.model.materialize(torch.device(DEV))
    save_policy_checkpoint(flow, tmp_path / "flow")
    tr = Trainer(plain, [], None, TrainingConfig(output_dir=str(tmp_path / "x"), max_steps=1))
    with pytest.raises(ValueError, match=r"fusion\.0\.weight is \(64, \d+\) in the checkpoint and \(64, \d+\) in this policy.*flow_prefix_max_delay"):
        tr._load_checkpoint(str(tmp_path / "flow"))
    plain.load_state_dict(prefix.widen_flow_state_dict(flow.state_dict(), K))
    plain.model._flow_sample_calls = flow.model._flow_sample_calls
    wide_chunk, flow_chunk = plain.select_action_chunk(img, st, task, DEV), flow.select_action_chunk(img, st, task, DEV)
    # the bar: 4 x the fp32 emulation's distance from float64 on the plain head, this observation and this noise (the sampler tests' rule)
    m = flow.model
    eng = m._engine()
    with torch.no_grad():
        pooled = m.features(flow.processor.prepare_images(img.unsqueeze(0), DEV), flow.processor.prepare_tasks(task, batch_size=1), device=DEV)
        states = flow.processor.prepare_states(st.unsqueeze(0), DEV).float()
        noise = eng.head_flow_prepare(torch.zeros(1, K * A), eng.head_saved(1), seed=m._flow_seed, offset=(1 << 62) + m._flow_sample_calls)
    torch.cuda.synchronize()
    p = {k: v.detach().cpu().clone() for k, v in eng.head_views(m._flat).items()}
    ref = fu.euler_sample(p, pooled.cpu(), states.cpu(), noise.cpu(), m.flow_steps, 6)
    emu = fu.worst_row_vs_rms(fu.euler_sample_fp32(p, pooled.cpu(), states.cpu(), noise.cpu(), m.flow_steps, 6), ref)
    for what, c_ in (("widened", wide_chunk), ("plain", flow_chunk)):
        err = fu.worst_row_vs_rms(c_.cpu().reshape(1, -1), ref)
        print(f"[prefix policy widening] {what}: error {err:.3e}, bar {4 * emu:.3e}")
        assert err <= 4 * emu
    for p_ in (pol, plain, back, flow):
        p_.model.backbone.engine().close()


def test_lerobot_plugin_resets_one_environment_under_prefix(monkeypatch):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    K, A, B, n, D = 4, 5, 3, 2, 2
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}

    def make(**kw):
        torch.manual_seed(3)
        cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=K, n_action_steps=n,
                       output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)
        return LRPolicy(cfg, action_head="flow", flow_time_dim=6, flow_steps=5, flow_seed=11, flow_prefix_max_delay=D, **kw).to(DEV)

    g = torch.Generator().manual_seed(4)
    batch = {"observation.images.top": torch.rand(B, 3, 64, 64, generator=g).to(DEV), "observation.state": torch.randn(B, 6, generator=g).to(DEV),
             "task": ["a", "b", "c"]}
    runs = []
    for reset_env in (None, 1):
        pol = make(rtc=True, rtc_method="prefix")
        acts, chunks = [], []
        for i in range(3 * n):
            if i == n and reset_env is not None:
                pol.model.rtc_reset(reset_env)                      # environment 1 starts a new episode: its next plan pins nothing
            prev = pol.last_chunk_normalised
            acts.append(pol.select_action(batch).clone())
            if i % n == 0:
                chunks.append((prev, pol.last_chunk_normalised))
        assert all(a.shape == (B, A) and bool(torch.isfinite(a).all()) for a in acts) and pol.model._flow_sample_calls == 3
        pins = min(D, K - n)
        for j, (prev, chunk) in enumerate(chunks[1:], 1):
            rows = [b for b in range(B) if not (reset_env == b and j == 1)]
            assert torch.equal(chunk[rows, :pins], prev[rows, n:n + pins])
            if reset_env is not None and j == 1:
                assert not torch.equal(chunk[reset_env, :pins], prev[reset_env, n:n + pins])
        runs.append(torch.stack(acts))
        if reset_env is None:
            left = pol.last_chunk_normalised[:, 1:]
            chunk = pol.predict_action_chunk(batch, inference_delay=1, prev_chunk_left_over=left)
            assert chunk.shape == (B, K, A) and torch.equal(chunk[:, :1], left[:, :1]) and not torch.equal(chunk[:, 1], left[:, 1])
            chunk = pol.predict_action_chunk(batch, prev_chunk_left_over=left)                 # no delay given: the policy's rtc_prefix_steps = D
            assert torch.equal(chunk[:, :D], left[:, :D]) and not torch.equal(chunk[:, D], left[:, D])
            with pytest.raises(ValueError, match="inference_delay"):
                pol.predict_action_chunk(batch, inference_delay=D + 1, prev_chunk_left_over=left)
            with pytest.raises(ValueError, match="execution_horizon"):
                pol.predict_action_chunk(batch, inference_delay=1, prev_chunk_left_over=left, execution_horizon=2)
        pol.model.backbone.engine().close()
    same, other = runs
    assert torch.equal(same[:, [0, 2]], other[:, [0, 2]])                         # the other two environments: bit for bit
    assert torch.equal(same[:n, 1], other[:n, 1]) and not torch.equal(same[n:2 * n, 1], other[n:2 * n, 1])
