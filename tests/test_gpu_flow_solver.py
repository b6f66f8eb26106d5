"""-m gpu: the flow head's higher-order integrators (fv_head_set_flow_solver; midpoint, Heun, RK4) in all three samplers -- each against its float64
Runge-Kutta reference (tests/flow_solver_util.py), the bit rules, the refusals, and through the policy on every sampling route.

Bars.  Samplers: worst row against the RMS row norm, at most 4 x the distance of the fp32 CPU emulation from float64 on the same case
(tests/test_flow_solver_host.py keeps that distance below 1e-4 for every case used here).  Bit rules: torch.equal.  action_error_per_dim:
test_gpu_loss_weights' per-dimension bar (1e-5 relative) plus what the sampler's bar allows an element to move (4 x emulation x the RMS row norm)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_prefix_util as pu  # noqa: E402
import flow_solver_util as su  # noqa: E402
import flow_util as fu  # noqa: E402
import rtc_util as ru  # noqa: E402
from gpu_util import DEV  # noqa: E402
from fastvla_hip import FastVLAEngine, _lib, arch  # noqa: E402
from fastvla_hip.rtc import prefix_weights  # noqa: E402

ENV = ("FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_SOLVER", "FASTVLA_RTC", "FASTVLA_RTC_METHOD", "FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "FASTVLA_FLOW_PREFIX_MAX_DELAY",
       "FASTVLA_FLOW_NOISE_DRAWS", "FASTVLA_FLOW_STEPS")


def _engine(name, B, solver=None, D=None, weights=None, flow=True):
    """a head-only engine in flow mode.  solver None: the handle never makes the call; D: prefix mode; weights: guidance configured"""
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=ds, action_dim=K * A, hidden_dim=hid, fusion_dim=fus, max_batch=max(B, 1))
    if flow:
        eng.set_head_flow(E)
    if D is not None:
        eng.set_head_flow_prefix(K, D)
    if weights is not None:
        eng.set_head_flow_guidance(weights, ru.BETA)
    if solver is not None:
        eng.set_head_flow_solver(solver)
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


def _check(tag, got, ref, emu):
    err = fu.worst_row_vs_rms(got.cpu(), ref)
    print(f"[{tag}] error {err:.3e}, fp32 emulation {emu:.3e}, error / bar {err / (4 * emu):.3f}")
    assert bool(torch.isfinite(got).all()) and err <= 4 * emu, (tag, err, emu)
    return err / (4 * emu)


# ------------------------------------------------------------------------------------------------------------------ 1. the plain sampler
@pytest.mark.parametrize("solver", su.HIGHER)
@pytest.mark.parametrize("B", su.BATCHES)
@pytest.mark.parametrize("name", su.HEADS)
def test_plain_sampler_matches_float64_reference(name, B, solver):
    c = fu.sampler_case(name, B)
    eng = _engine(name, B, solver)
    flat = _flat(eng, c["p"])
    pooled, states = c["pooled"].to(DEV), c["states"].to(DEV)
    worst = 0.0
    for io in (False, True):
        _set_io(eng, c["stats"], io)
        for N in su.STEPS:
            act = eng.head_flow_sample(flat, pooled, states, steps=N, noise=c["noise"])
            torch.cuda.synchronize()
            ref, emu = su.plain_refs(name, B, N, io, solver)
            worst = max(worst, _check(f"solver plain {solver} {name} B={B} N={N} io={int(io)}", act, ref, emu))
    print(f"[solver plain {solver} {name} B={B}] worst error / bar {worst:.3f}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the prefix sampler
@pytest.mark.parametrize("solver", su.HIGHER)
@pytest.mark.parametrize("B", su.BATCHES)
@pytest.mark.parametrize("name", su.HEADS)
def test_prefix_sampler_matches_float64_reference_and_pins(name, B, solver):
    c = su.prefix_case(name, B)
    K, A = c["dims"][4], c["dims"][5]
    da, D = K * A, c["D"]
    eng = _engine(name, B, solver, D=D)
    flat = _flat(eng, c["p"])
    pooled, states, prev, delays = c["pooled"].to(DEV), c["states"].to(DEV), c["prev"].to(DEV), torch.from_numpy(c["delays"]).to(DEV)
    worst = 0.0
    for shift in su.PREFIX_SHIFTS(K):
        pin = pu.pinned_steps(c["delays"], D, K, shift)
        pinned = torch.from_numpy(pu.mask_ref(pin, K)).bool().repeat_interleave(A, dim=1)
        src = torch.zeros(B, da)
        src[:, :da - shift * A] = c["prev"][:, shift * A:]                 # prev read `shift` steps ahead
        # what must never be read: everything of prev that is not the source of a pinned element -- NaN and +-inf there change no bit
        bad = c["prev"].clone()
        unread = torch.ones(B, da, dtype=torch.bool)
        for b in range(B):
            unread[b, shift * A:shift * A + int(pin[b]) * A] = False
        bad[unread] = torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat(da * B)[:int(unread.sum())]
        for io in (False, True):
            _set_io(eng, c["stats"], io)
            for N in su.STEPS:
                act, chunk = eng.head_flow_sample_prefix(flat, pooled, states, prev, delays, shift=shift, steps=N, noise=c["noise"])
                torch.cuda.synchronize()
                a64, c64, ea, ec = su.prefix_refs(name, B, N, io, shift, solver)
                tag = f"solver prefix {solver} {name} B={B} shift={shift} N={N} io={int(io)}"
                worst = max(worst, _check(tag + " actions", act, a64, ea), _check(tag + " chunk_out", chunk, c64, ec))
                assert bool(pinned.any()) and torch.equal(chunk.cpu()[pinned], src[pinned])          # pinned steps leave as the bits of prev
                act2, chunk2 = eng.head_flow_sample_prefix(flat, pooled, states, bad.to(DEV), delays, shift=shift, steps=N, noise=c["noise"])
                assert torch.equal(act2, act) and torch.equal(chunk2, chunk)
    print(f"[solver prefix {solver} {name} B={B}] worst error / bar {worst:.3f}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the guided sampler
@pytest.mark.parametrize("solver", su.HIGHER)
@pytest.mark.parametrize("B", su.BATCHES)
@pytest.mark.parametrize("name", su.HEADS)
def test_guided_sampler_matches_float64_reference(name, B, solver):
    c = ru.rtc_case(name, B)
    K = c["dims"][4]
    eng = _engine(name, B, solver, weights=prefix_weights(K, 0, 1, "exp"))
    flat = _flat(eng, c["p"])
    pooled, states, prev = c["pooled"].to(DEV), c["states"].to(DEV), c["prev"].to(DEV)
    worst = 0.0
    for schedule, which in su.GUIDED_CONFIGS:
        d, s, shift = ru.rtc_config(K, which)
        eng.set_head_flow_guidance(prefix_weights(K, d, s, schedule), ru.BETA)
        for io in (False, True):
            _set_io(eng, c["stats"], io)
            for N in su.STEPS:
                act, chunk = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, steps=N, noise=c["noise"])
                torch.cuda.synchronize()
                a64, c64, ea, ec = su.guided_refs(name, B, N, io, schedule, which, solver)
                tag = f"solver guided {solver} {name} B={B} {schedule} {which} N={N} io={int(io)}"
                worst = max(worst, _check(tag + " actions", act, a64, ea), _check(tag + " chunk_out", chunk, c64, ec))
    print(f"[solver guided {solver} {name} B={B}] worst error / bar {worst:.3f}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4. bit rules
@pytest.mark.parametrize("name,B", [("awkward", 9), ("larger", 67), ("larger", 1)])
def test_euler_on_a_handle_with_the_rows_is_the_handle_that_never_asked(name, B):
    c = su.prefix_case(name, B)
    K, D = c["dims"][4], c["D"]
    w = prefix_weights(K, 1, 1, "exp")
    never, back = _engine(name, B, None, D=D, weights=w), _engine(name, B, "rk4", D=D, weights=w)
    assert back.workspace_bytes(B, 1, False) > never.workspace_bytes(B, 1, False)
    pooled, states, prev, delays = c["pooled"].to(DEV), c["states"].to(DEV), c["prev"].to(DEV), torch.from_numpy(c["delays"]).to(DEV)
    outs = {}
    for key, eng in (("never", never), ("back", back)):
        flat = _flat(eng, c["p"])
        kw = dict(steps=4, noise=c["noise"])
        if key == "back":
            rk = eng.head_flow_sample(flat, pooled, states, **kw)          # the higher-order path runs first and leaves its rows behind
            eng.set_head_flow_solver("euler")
        outs[key] = (eng.head_flow_sample(flat, pooled, states, **kw), *eng.head_flow_sample_prefix(flat, pooled, states, prev, delays, shift=1, **kw),
                     *eng.head_flow_sample_guided(flat, pooled, states, prev, shift=1, **kw))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs["never"], outs["back"])) and not torch.equal(rk, outs["back"][0])
    never.close(), back.close()


@pytest.mark.parametrize("solver", su.HIGHER)
@pytest.mark.parametrize("name,B", [("awkward", 9), ("larger", 67), ("larger", 1)])
def test_bit_rules(name, B, solver):
    c = ru.rtc_case(name, B)
    K, A = c["dims"][4], c["dims"][5]
    da = K * A
    d = shift = max(1, K // 3)
    w = prefix_weights(K, d, d + 1, "exp")
    eng = _engine(name, B, solver, weights=w)
    flat = _flat(eng, c["p"])
    pooled, states, prev, noise = c["pooled"].to(DEV), c["states"].to(DEV), c["prev"].to(DEV), c["noise"]
    for io in (False, True):
        _set_io(eng, c["stats"], io)
        for N in (1, 4):
            kw = dict(steps=N, noise=noise)
            plain = eng.head_flow_sample(flat, pooled, states, **kw)
            assert torch.equal(plain, eng.head_flow_sample(flat, pooled, states, **kw))                          # two calls agree
            guided, gchunk = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, **kw)
            again, cagain = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, **kw)
            assert torch.equal(guided, again) and torch.equal(gchunk, cagain) and not torch.equal(guided, plain)
            # nothing guides: the plain sampler's bits for the same solver
            zeros = torch.zeros(B, dtype=torch.int32, device=DEV)
            a_mask, c_mask = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, row_mask=zeros, **kw)
            a_shift, _ = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=K, **kw)
            eng.set_head_flow_guidance([0.0] * K, ru.BETA)
            a_zero, _ = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, **kw)
            eng.set_head_flow_guidance(w, ru.BETA)
            assert torch.equal(a_mask, plain) and torch.equal(a_shift, plain) and torch.equal(a_zero, plain)
            if not io:
                assert torch.equal(c_mask, plain)
            # a mixed mask gives the respective rows
            mask = (torch.arange(B) % 2 == 0).to(torch.int32)
            mixed, _ = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, row_mask=mask, **kw)
            on = mask.bool().to(DEV)
            assert torch.equal(mixed[on], guided[on]) and torch.equal(mixed[~on], plain[~on])
            # NaN in one row's noise reaches no other row, in either sampler
            if B > 1:
                bad = noise.clone()
                bad[1, da // 2] = float("nan")
                hp = eng.head_flow_sample(flat, pooled, states, steps=N, noise=bad)
                hg, _ = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, steps=N, noise=bad)
                keep = torch.arange(B) != 1
                assert bool(torch.isnan(hp[1]).any()) and torch.equal(hp[keep], plain[keep]) and torch.equal(hg[keep], guided[keep])
    eng.close()
    # a prefix-mode handle: no delays pin nothing and add no mask column -- the plain sampler's bits for the same solver, whatever the shift
    pc = su.prefix_case(name, B)
    eng = _engine(name, B, solver, D=pc["D"])
    flat = _flat(eng, pc["p"])
    none = torch.zeros(B, dtype=torch.int32, device=DEV)
    for io in (False, True):
        _set_io(eng, pc["stats"], io)
        for N in (1, 4):
            plain = eng.head_flow_sample(flat, pooled, states, steps=N, noise=noise).clone()
            for sh in (0, 2, K):
                a_none, c_none = eng.head_flow_sample_prefix(flat, pooled, states, prev, none, shift=sh, steps=N, noise=noise)
                assert torch.equal(a_none, plain) and (io or torch.equal(c_none, plain)), (io, N, sh)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_actions_untouched():
    from gpu_util import stream
    name, B = "awkward", 5
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    c = fu.sampler_case(name, 9)
    fresh, asked, late = _engine(name, B), _engine(name, B), _engine(name, B)
    L = fresh.lib
    reg = _engine(name, B, flow=False)
    assert L.fv_head_set_flow_solver(reg.h, 1) == -2 and L.fv_head_set_flow_solver(None, 1) == -1                 # flow mode off: FV_ERR_STATE
    reg.close()
    # a handle that never asked reports what a fresh flow handle reports; asking grows it and it stays grown under Euler
    n0, n1 = fresh.workspace_bytes(B, 1, False), asked.workspace_bytes(B, 1, False)
    assert n0 == n1
    assert L.fv_head_set_flow_solver(asked.h, _lib.FLOW_SOLVERS["heun"]) == 0
    n2 = asked.workspace_bytes(B, 1, False)
    assert n2 >= n1 and fresh.workspace_bytes(B, 1, False) == n0      # (this head's backward scratch is the larger part of the plan: the two rows fit inside)
    guided = _engine(name, B, weights=prefix_weights(K, 1, 1, "exp"))      # the guided sampler's rows are the largest part: the two rows add to them
    g0 = guided.workspace_bytes(B, 1, False)
    guided.set_head_flow_solver("midpoint")
    assert guided.workspace_bytes(B, 1, False) >= g0 + 2 * B * da * 4
    guided.close()
    assert L.fv_head_set_flow_solver(asked.h, 0) == 0 and asked.workspace_bytes(B, 1, False) == n2
    assert L.fv_head_set_flow_solver(asked.h, _lib.FLOW_SOLVERS["heun"]) == 0
    flat = _flat(asked, c["p"])
    pooled, states, noise = c["pooled"][:B].to(DEV), c["states"][:B].to(DEV), c["noise"][:B].to(DEV).contiguous()
    out = torch.full((B, da), float("nan"), device=DEV)

    def call(eng, fl):
        return L.fv_head_flow_sample(eng.h, fl.data_ptr(), pooled.data_ptr(), states.data_ptr(), B, 2, noise.data_ptr(), 0, 0, out.data_ptr(), stream())

    # an unknown id: FV_ERR_ARG, nothing changed (the solver stays Heun)
    asked.ensure_workspace(B, 1, False)
    want = asked.head_flow_sample(flat, pooled, states, steps=2, noise=noise)
    for bad in (-1, 4, 99):
        assert L.fv_head_set_flow_solver(asked.h, bad) == -1 and b"solver" in L.fv_last_error(asked.h)
    assert call(asked, flat) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # the first higher-order call after fv_bind_workspace: FV_ERR_STATE; Euler is accepted at any time, and the handle samples as ever
    late.ensure_workspace(B, 1, False)
    flat_l = _flat(late, c["p"])
    ref = late.head_flow_sample(flat_l, pooled, states, steps=2, noise=noise)
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    for sid in (1, 2, 3):
        assert L.fv_head_set_flow_solver(late.h, sid) == -2 and b"fv_bind_workspace" in L.fv_last_error(late.h)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                                                    # refusals enqueue nothing
    assert L.fv_head_set_flow_solver(late.h, 0) == 0 and late.workspace_bytes(B, 1, False) == n0
    assert torch.equal(late.head_flow_sample(flat_l, pooled, states, steps=2, noise=noise), ref)
    # later calls switch freely among all four on the handle that asked in time
    for nm in ("rk4", "euler", "midpoint", "heun"):
        asked.set_head_flow_solver(nm)
        assert asked.head_flow_solver == nm and bool(torch.isfinite(asked.head_flow_sample(flat, pooled, states, steps=2, noise=noise)).all())
    with pytest.raises(ValueError):
        asked.set_head_flow_solver("rk5")
    # fv_head_set_flow(NULL) returns the solver to Euler (a handle without a bound workspace)
    assert L.fv_head_set_flow_solver(fresh.h, 3) == 0
    fresh.set_head_flow(None)
    fresh.set_head_flow(E)
    plain = _engine(name, B)
    fl_f, fl_p = _flat(fresh, c["p"]), _flat(plain, c["p"])
    assert torch.equal(fresh.head_flow_sample(fl_f, pooled, states, steps=3, noise=noise), plain.head_flow_sample(fl_p, pooled, states, steps=3, noise=noise))
    for e in (fresh, asked, late, plain):
        e.close()


# ------------------------------------------------------------------------------------------------------------------ 6. the policy
def _policy(K, n_steps, seed=0, **kw):
    from vla_fastvlm.fastvla.configuration_fastvla import FastVLAConfig
    from vla_fastvlm.fastvla.modeling_fastvla import FastVLAPolicy
    torch.manual_seed(seed)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K, n_action_steps=n_steps,
                         action_head="flow", flow_time_dim=6, flow_seed=77, **kw).to(DEV)


def _policy_inputs(pol, img, st, task, offset):
    """the policy's own pooled feature, prepared state, head and the noise it draws at `offset` of its flow seed (read back: u = eps - 0)"""
    m = pol.model
    eng = m._engine()
    K, A = m.chunk_size, pol.config.action_dim
    with torch.no_grad():
        images = img if img.ndim == 4 else img.unsqueeze(0)
        pooled = m.features(pol.processor.prepare_images(images, DEV), pol.processor.prepare_tasks(task, batch_size=images.shape[0]), device=DEV)
        states = pol.processor.prepare_states(st if st.ndim == 2 else st.unsqueeze(0), DEV).float()
        noise = eng.head_flow_prepare(torch.zeros(images.shape[0], K * A), eng.head_saved(images.shape[0]), seed=m._flow_seed, offset=offset)
    torch.cuda.synchronize()
    p = {k: v.detach().cpu().clone() for k, v in eng.head_views(m._flat).items()}
    return p, pooled.cpu(), states.cpu(), noise.cpu()


def test_policy_samples_with_the_solver_on_every_route(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    K, n, A, E = 8, 3, 14, 6
    g = torch.Generator().manual_seed(5)
    img, st, task = torch.rand(3, 72, 96, generator=g).to(DEV), torch.randn(14, generator=g).to(DEV), "open drawer"
    kw = dict(flow_solver="heun", flow_steps=3)
    # --- select_action_chunk: the plain sampler
    pol, euler = _policy(K, n, **kw), _policy(K, n, flow_steps=3)
    assert pol.flow_solver == "heun" and euler.flow_solver == "euler"
    got = pol.select_action_chunk(img, st, task, DEV)
    p, pooled, states, noise = _policy_inputs(pol, img, st, task, (1 << 62) + 1)
    ref = su.rk_sample(p, pooled, states, noise, 3, E, "heun")
    emu = fu.worst_row_vs_rms(su.rk_sample_fp32(p, pooled, states, noise, 3, E, "heun"), ref)
    _check("solver policy chunk", got.reshape(1, -1), ref, emu)
    # switched back to Euler, the policy reproduces an Euler policy's chunk bit for bit (same weights: the same seed built both)
    pol.flow_solver = "euler"
    e1 = euler.select_action_chunk(img, st, task, DEV)
    pol.model._flow_sample_calls = euler.model._flow_sample_calls - 1
    assert torch.equal(pol.select_action_chunk(img, st, task, DEV), e1) and not torch.equal(e1, got)
    with pytest.raises(ValueError, match="build the policy with flow_solver"):
        euler.flow_solver = "heun"
    for q in (pol, euler):
        q.model.backbone.engine().close()
    # --- rtc, guidance: the second plan is guided by the first
    pol = _policy(K, n, rtc=True, **kw)
    w = prefix_weights(K, 0, n, "exp")
    first = pol.select_action_chunk(img, st, task, DEV)
    prev = pol.last_chunk_normalised.cpu().reshape(1, -1)
    second = pol.select_action_chunk(img, st, task, DEV)
    p, pooled, states, noise = _policy_inputs(pol, img, st, task, (1 << 62) + 2)
    Y, W = ru.targets(prev, w, K, A, 0)
    args = (p, pooled, states, noise, 3, E, Y, W, pol.rtc["max_guidance_weight"], "heun")
    _, c64 = su.guided_rk(*args)
    _, c32 = su.guided_rk(*args, fp32=True)
    _check("solver policy rtc guidance", second.reshape(1, -1), c64, fu.worst_row_vs_rms(c32, c64))
    assert not torch.equal(first, second)
    pol.model.backbone.engine().close()
    # --- rtc, prefix: the second plan pins D steps of the first
    D = 2
    pol = _policy(K, n, rtc=True, rtc_method="prefix", flow_prefix_max_delay=D, **kw)
    pol.select_action_chunk(img, st, task, DEV)
    prev = pol.last_chunk_normalised.cpu().reshape(1, -1)
    second = pol.select_action_chunk(img, st, task, DEV)
    p, pooled, states, noise = _policy_inputs(pol, img, st, task, (1 << 62) + 2)
    args = (p, pooled, states, noise, prev, np.array([D], dtype=np.int32), 0, 3, E, K, D, "heun")
    _, c64 = su.prefix_rk(*args)
    _, c32 = su.prefix_rk(*args, fp32=True)
    _check("solver policy rtc prefix", second.reshape(1, -1), c64, fu.worst_row_vs_rms(c32, c64))
    assert torch.equal(second.reshape(1, -1)[:, :D * A].cpu(), prev[:, :D * A])
    pol.model.backbone.engine().close()


@pytest.mark.parametrize("prefix", [False, True])
def test_policy_action_error_per_dim_samples_with_the_solver(monkeypatch, prefix):
    """The noise is the flow seed's at offset 2^63 (flow_util.draw_normals is its float64 form: the device's values are checked against it within its own
    per-element bar); the float64 reference solver then runs from the device's values, so that the sampler's bar is the only arithmetic between the two."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    K, A, E, B = 8, 14, 6, 3
    pol = _policy(K, 1, flow_solver="rk4", flow_steps=2, **(dict(flow_prefix_max_delay=2) if prefix else {}))
    batch = pu.policy_batch(B, K, seed=3, device=DEV)
    err = pol.action_error_per_dim(batch)
    calls = pol.model._flow_sample_calls
    assert calls == 0 and torch.equal(pol.action_error_per_dim(batch), err)                  # repeatable; the sampling counter does not advance
    p, pooled, states, noise = _policy_inputs(pol, batch["images"], batch["states"], batch["tasks"], su.SAMPLE_OFFSET_ERROR)
    n64, nbar = fu.draw_normals(B, K * A, pol.model._flow_seed, su.SAMPLE_OFFSET_ERROR)
    assert bool((np.abs(noise.double().numpy() - n64) <= nbar).all())
    if prefix:      # a prefix-width head samples with m = 0
        args = (p, pooled, states, noise, torch.zeros(B, K * A), np.zeros(B, dtype=np.int32), 0, 2, E, K, 2, "rk4")
        _, s64 = su.prefix_rk(*args)
        _, s32 = su.prefix_rk(*args, fp32=True)
    else:
        s64 = su.rk_sample(p, pooled, states, noise, 2, E, "rk4")
        s32 = su.rk_sample_fp32(p, pooled, states, noise, 2, E, "rk4")
    emu = fu.worst_row_vs_rms(s32, s64)
    valid = ~batch["action_is_pad"].cpu().numpy()
    tgt = batch["actions"].cpu().double().numpy()
    ref = torch.from_numpy(np.abs(s64.view(B, K, A).numpy() - tgt)[valid].mean(axis=0))
    bar = 1e-5 * ref + 4 * emu * float(s64.norm(dim=1).pow(2).mean().sqrt())
    print(f"[solver policy action error prefix={int(prefix)}] worst error / bar {float(((err.cpu().double() - ref).abs() / bar).max()):.3f}, fp32 emulation {emu:.3e}")
    assert err.shape == (A,) and bool(((err.cpu().double() - ref).abs() <= bar).all())
    # the next sampled chunk is what it would have been without the metric
    img, st = batch["images"][0], batch["states"][0]
    nxt = pol.select_action_chunk(img, st, batch["tasks"][0], DEV)
    pol.model._flow_sample_calls = 0
    pol.reset()
    assert torch.equal(pol.select_action_chunk(img, st, batch["tasks"][0], DEV), nxt)
    # another solver or step count is another sample
    pol.flow_solver = "euler"
    assert not torch.equal(pol.action_error_per_dim(batch), err)
    pol.model.backbone.engine().close()


def test_lerobot_plugin_samples_with_the_solver(monkeypatch):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    K, A, B = 4, 5, 3
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}

    def make(**kw):
        torch.manual_seed(3)
        cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=K, n_action_steps=2,
                       output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)
        return LRPolicy(cfg, action_head="flow", flow_time_dim=6, flow_steps=3, flow_seed=11, **kw).to(DEV)

    g = torch.Generator().manual_seed(4)
    batch = {"observation.images.top": torch.rand(B, 3, 64, 64, generator=g).to(DEV), "observation.state": torch.randn(B, 6, generator=g).to(DEV),
             "task": ["a", "b", "c"]}
    pol, euler = make(flow_solver="midpoint"), make()
    got = pol.predict_action_chunk(batch)
    m = pol.model
    eng = m._engine()
    with torch.no_grad():
        images, states, tasks = pol._prepare_inputs(batch)
        pooled = m.features(images, tasks, device=DEV)
        noise = eng.head_flow_prepare(torch.zeros(B, K * A), eng.head_saved(B), seed=m._flow_seed, offset=(1 << 62) + 1)
    torch.cuda.synchronize()
    p = {k: v.detach().cpu().clone() for k, v in eng.head_views(m._flat).items()}
    args = (p, pooled.cpu(), states.float().cpu(), noise.cpu(), 3, 6, "midpoint")
    ref = su.rk_sample(*args)
    _check("solver plugin chunk", got.reshape(B, -1), ref, fu.worst_row_vs_rms(su.rk_sample_fp32(*args), ref))
    e1 = euler.predict_action_chunk(batch)
    pol.flow_solver = "euler"
    pol.model._flow_sample_calls = 0
    assert torch.equal(pol.predict_action_chunk(batch), e1) and not torch.equal(e1, got)
    for q in (pol, euler):
        q.model.backbone.engine().close()
