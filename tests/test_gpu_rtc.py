"""-m gpu: real-time chunking of the flow head -- the guided step's vector-Jacobian product against float64 autograd, the guided sampler against the float64
reference, the bit rules that make an unguided row of a guided call the unguided sampler's row, the prefix property, refusals, and the policy surfaces.

Bars.  VJP and sampler: worst row against the RMS row norm (flow_util.worst_row_vs_rms), at most 4 x the distance of the fp32 CPU emulation from float64
for the same case (the factor covers another summation order; tests/test_rtc_host.py keeps that distance below 1e-4).  The measured value is printed beside
the bar.  Prefix property: the host test's condition, on the device's output."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_util as fu  # noqa: E402
import rtc_util as ru  # noqa: E402
from gpu_util import DEV  # noqa: E402
from fastvla_hip import FastVLAEngine, _lib, arch  # noqa: E402
from fastvla_hip.rtc import prefix_weights  # noqa: E402


def _engine(name, B, weights=None, beta=ru.BETA, flow=True):
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=ds, action_dim=K * A, hidden_dim=hid, fusion_dim=fus, max_batch=max(B, 1))
    if flow:
        eng.set_head_flow(E)
    if weights is not None:
        eng.set_head_flow_guidance(weights, beta)
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


def _inputs(case):
    return case["pooled"].to(DEV), case["states"].to(DEV)


# ------------------------------------------------------------------------------------------------------------------ 1. the VJP alone
@pytest.mark.parametrize("B", fu.SAMPLER_BATCHES)
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_vjp_matches_float64_autograd(name, B):
    from gpu_util import lib, stream
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    case = ru.rtc_case(name, B)
    eng = _engine(name, B)
    flat = _flat(eng, case["p"])
    freq = torch.from_numpy(fu.flow_freqs(E)).to(DEV)
    pooled, states = _inputs(case)
    x = case["noise"]
    g = torch.Generator().manual_seed(90 + B)
    dense = torch.randn(B, da, generator=g)
    first = torch.zeros(B, da)
    first[:, :A] = dense[:, :A]
    scr = torch.zeros(1 << 21, device=DEV)
    xd = x.to(DEV)
    worst = 0.0
    for t in (1.0, 0.5, float(np.float32(0.1))):
        for label, om in (("dense", dense), ("first step", first)):
            omd = om.to(DEV)
            v, jt = torch.full((B, da), float("nan"), device=DEV), torch.full((B, da), float("nan"), device=DEV)
            _lib.check(lib().fv_op_flow_vjp(feat, ds, da, hid, fus, E, freq.data_ptr(), flat.data_ptr(), pooled.data_ptr(), states.data_ptr(), B,
                                            xd.data_ptr(), t, omd.data_ptr(), v.data_ptr(), jt.data_ptr(), scr.data_ptr(), scr.numel(), stream()),
                       "fv_op_flow_vjp")
            torch.cuda.synchronize()
            v64, jt64 = ru.vjp_ref(case["p"], case["pooled"], case["states"], x, t, om, E)
            v32, jt32 = ru.vjp_ref(case["p"], case["pooled"], case["states"], x, t, om, E, fp32=True)
            for what, got, ref, emu in (("v", v, v64, v32), ("J^T omega", jt, jt64, jt32)):
                bar = 4 * fu.worst_row_vs_rms(emu, ref)
                err = fu.worst_row_vs_rms(got.cpu(), ref)
                worst = max(worst, err / bar)
                print(f"[rtc vjp {name} B={B} t={t:.2f} {label}] {what}: error {err:.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}")
                assert bool(torch.isfinite(got).all()) and err <= bar
    print(f"[rtc vjp {name} B={B}] worst error / bar {worst:.3f}")
    # the scratch check names the count, and nothing runs
    assert lib().fv_op_flow_vjp(feat, ds, da, hid, fus, E, freq.data_ptr(), flat.data_ptr(), pooled.data_ptr(), states.data_ptr(), B, xd.data_ptr(), 1.0,
                                omd.data_ptr(), v.data_ptr(), jt.data_ptr(), scr.data_ptr(), 16, stream()) == -1
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the guided sampler against float64
@pytest.mark.parametrize("B", fu.SAMPLER_BATCHES)
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_guided_sampler_matches_float64_reference(name, B):
    case = ru.rtc_case(name, B)
    K = case["dims"][4]
    eng = _engine(name, B, weights=prefix_weights(K, 0, 1, "exp"))
    flat = _flat(eng, case["p"])
    pooled, states = _inputs(case)
    prev = case["prev"].to(DEV)
    worst = 0.0
    for schedule in ("exp", "zeros"):
        for which in ru.RTC_CONFIGS:
            d, s, shift = ru.rtc_config(K, which)
            eng.set_head_flow_guidance(prefix_weights(K, d, s, schedule), ru.BETA)
            for io in (False, True):
                _set_io(eng, case["stats"], io)
                for N in fu.SAMPLER_STEPS:
                    act, chunk = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, steps=N, noise=case["noise"])
                    torch.cuda.synchronize()
                    a64, c64, ea, ec = ru.guided_refs(name, B, N, io, schedule, which)
                    for what, got, ref, emu in (("actions", act, a64, ea), ("chunk_out", chunk, c64, ec)):
                        err = fu.worst_row_vs_rms(got.cpu(), ref)
                        # (a case whose every live weight is 0 is the unguided sampler: its emulation distance is the bar all the same)
                        worst = max(worst, err / (4 * emu))
                        print(f"[rtc sampler {name} B={B} {schedule} {which} N={N} io={int(io)}] {what}: error {err:.3e}, fp32 emulation {emu:.3e}, "
                              f"error / bar {err / (4 * emu):.3f}")
                        assert bool(torch.isfinite(got).all()) and err <= 4 * emu
    print(f"[rtc sampler {name} B={B}] worst error / bar {worst:.3f}")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 3. bit rules
@pytest.mark.parametrize("name,B", [("awkward", 9), ("larger", 67), ("larger", 1)])
def test_bit_rules(name, B):
    case = ru.rtc_case(name, B)
    K, A = case["dims"][4], case["dims"][5]
    da = K * A
    d = shift = max(1, K // 3)
    s = d + 1              # one more free step than the shift: step K - 1 - shift has weight 0 AND a target (the last row of prev)
    w = prefix_weights(K, d, s, "exp")
    eng = _engine(name, B, weights=w)
    flat = _flat(eng, case["p"])
    pooled, states = _inputs(case)
    prev, noise = case["prev"].to(DEV), case["noise"]
    for io in (False, True):
        _set_io(eng, case["stats"], io)
        for N in (1, 4):
            kw = dict(steps=N, noise=noise)
            plain = eng.head_flow_sample(flat, pooled, states, **kw)
            guided, gchunk = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, **kw)
            again, _ = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, **kw)
            assert torch.equal(guided, again) and not torch.equal(guided, plain)                                      # two calls: the same bits
            # nothing guides: the unguided sampler's bits
            zeros = torch.zeros(B, dtype=torch.int32, device=DEV)
            a_mask, c_mask = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, row_mask=zeros, **kw)
            a_shift, _ = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=K, **kw)
            assert torch.equal(a_mask, plain) and torch.equal(a_shift, plain)
            eng.set_head_flow_guidance([0.0] * K, ru.BETA)
            a_zero, _ = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, **kw)
            eng.set_head_flow_guidance(w, ru.BETA)
            assert torch.equal(a_zero, plain)
            # chunk_out, then the folded statistics: actions within 1 ulp per element
            st = case["stats"]
            want = (gchunk.cpu().double() * st["action_std"].double() + st["action_mean"].double()) if io else gchunk.cpu().double()
            assert bool(((guided.cpu().double() - want).abs() <= torch.from_numpy(fu.ulp32(want.numpy()))).all())
            if not io:
                assert torch.equal(c_mask, plain)
            # a mixed mask: masked rows are the unguided rows, the others the all-guided call's
            mask = (torch.arange(B) % 2 == 0).to(torch.int32)
            mixed, _ = eng.head_flow_sample_guided(flat, pooled, states, prev, shift=shift, row_mask=mask, **kw)
            on = mask.bool()
            assert torch.equal(mixed[on.to(DEV)], guided[on.to(DEV)]) and torch.equal(mixed[(~on).to(DEV)], plain[(~on).to(DEV)])
            # NaN / inf in prev where it must not be read: weight 0 (the last s steps of the target), beyond the shift (the first `shift` steps of prev),
            # a masked row -- no bit changes
            bad = case["prev"].clone().view(B, K, A)
            bad[:, :shift] = float("nan")                      # never a target: Y[k] = prev[k + shift]
            bad[:, K - 1] = float("inf")                       # the target of step K - 1 - shift = K - s, whose weight is 0
            assert w[K - 1 - shift] == 0.0 and w[K - 2 - shift] > 0.0
            if B > 1:
                bad[1] = float("-inf")                         # row 1 is masked in `mask`
            poisoned, _ = eng.head_flow_sample_guided(flat, pooled, states, bad.view(B, da).to(DEV), shift=shift, row_mask=mask, **kw)
            assert torch.equal(poisoned, mixed)
            # NaN under a positive weight reaches its own row only
            bad = case["prev"].clone().view(B, K, A)
            bad[0, shift, 0] = float("nan")                    # target of step 0, weight w[0] = 1
            hit, _ = eng.head_flow_sample_guided(flat, pooled, states, bad.view(B, da).to(DEV), shift=shift, **kw)
            assert bool(torch.isnan(hit[0]).any()) and torch.equal(hit[1:], guided[1:])
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the prefix property on the device
@pytest.mark.parametrize("B", fu.SAMPLER_BATCHES)
@pytest.mark.parametrize("name", ["awkward", "larger"])
def test_hard_prefix_converges_on_the_device(name, B):
    case = ru.rtc_case(name, B)
    K, A = case["dims"][4], case["dims"][5]
    d = s = max(1, K // 3)
    eng = _engine(name, B, weights=prefix_weights(K, d, s, "exp"))
    flat = _flat(eng, case["p"])
    pooled, states = _inputs(case)
    Y, _ = ru.targets(case["prev"], np.ones(K), K, A, 0)
    for N in (4, 10):
        plain = eng.head_flow_sample(flat, pooled, states, steps=N, noise=case["noise"])
        _, chunk = eng.head_flow_sample_guided(flat, pooled, states, case["prev"].to(DEV), shift=0, steps=N, noise=case["noise"])
        torch.cuda.synchronize()
        got, free = ru.prefix_distance(chunk.cpu(), Y, d, A), ru.prefix_distance(plain.cpu(), Y, d, A)
        print(f"[rtc prefix {name} B={B} N={N}] hard prefix {got:.4f} vs unguided {free:.3f} (ratio {got / free:.4f}, bar 0.1)")
        assert got <= 0.1 * free
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5. refusals, off means off
def test_refusals_and_off_means_off():
    name, B = "awkward", 5
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    case = ru.rtc_case(name, 9)
    fresh, seen = _engine(name, B), _engine(name, B)
    L = seen.lib
    w = (C.c_float * K)(*prefix_weights(K, 1, 1, "exp"))
    reg = _engine(name, B, flow=False)
    assert L.fv_head_set_flow_guidance(reg.h, K, w, 5.0) == -2 and L.fv_head_set_flow_guidance(None, K, w, 5.0) == -1        # flow mode off: FV_ERR_STATE
    reg.close()
    # every bad configuration: FV_ERR_ARG, nothing changed (guidance stays unconfigured: the guided call answers FV_ERR_STATE)
    for chunk, vals, beta in ((0, [1, 1, 1], 5.0), (-1, [1, 1, 1], 5.0), (2, [1, 1], 5.0), (4, [1, 1, 1, 1], 5.0), (K, [1, -0.5, 0], 5.0),
                              (K, [1, float("nan"), 0], 5.0), (K, [float("inf"), 1, 0], 5.0), (K, [1, 1, 0], 0.0), (K, [1, 1, 0], -1.0),
                              (K, [1, 1, 0], float("nan")), (K, [1, 1, 0], float("inf"))):
        assert L.fv_head_set_flow_guidance(seen.h, chunk, (C.c_float * len(vals))(*vals), beta) == -1, (chunk, vals, beta)
    flat = _flat(seen, {k: v for k, v in case["p"].items()})
    pooled, states = torch.zeros(B, feat, device=DEV), torch.zeros(B, ds, device=DEV)
    prev = torch.zeros(B, da, device=DEV)
    out, cout = torch.full((B, da), float("nan"), device=DEV), torch.full((B, da), float("nan"), device=DEV)
    args = (flat.data_ptr(), pooled.data_ptr(), states.data_ptr())

    def call(h, a=args, b=B, n=10, pv=prev.data_ptr(), sh=1, o=out.data_ptr()):
        return L.fv_head_flow_sample_guided(h, *a, b, n, None, 0, 0, pv, sh, None, o, cout.data_ptr(), None)

    assert call(seen.h) == -2 and b"fv_head_set_flow_guidance" in L.fv_last_error(seen.h)               # not configured
    # a handle that never configures guidance reports what a second handle of the same mode reports; configuring grows it
    n0, n1, n2 = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert L.fv_workspace_bytes(fresh.h, B, 1, 0, C.byref(n0)) == 0 and L.fv_workspace_bytes(seen.h, B, 1, 0, C.byref(n1)) == 0 and n0.value == n1.value
    assert L.fv_head_set_flow_guidance(seen.h, K, w, 5.0) == 0
    assert L.fv_workspace_bytes(seen.h, B, 1, 0, C.byref(n2)) == 0 and n2.value > n1.value
    assert L.fv_workspace_bytes(fresh.h, B, 1, 0, C.byref(n0)) == 0 and n0.value == n1.value
    assert call(seen.h) == -2 and b"fv_bind_workspace" in L.fv_last_error(seen.h)                       # no workspace bound yet
    seen.ensure_workspace(B, 1, False)
    assert call(None) == -1
    assert call(seen.h, n=0) == -1 and call(seen.h, n=-2) == -1
    assert call(seen.h, b=0) == -1 and call(seen.h, b=B + 1) == -1
    assert call(seen.h, sh=-1) == -1 and call(seen.h, sh=K + 1) == -1
    assert call(seen.h, pv=None) == -1 and call(seen.h, o=None) == -1
    assert call(seen.h, a=(None, args[1], args[2])) == -1 and call(seen.h, a=(args[0], None, args[2])) == -1 and call(seen.h, a=(args[0], args[1], None)) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(cout).all())                                # a refused call enqueues nothing
    assert call(seen.h) == 0 and call(seen.h, sh=0) == 0 and call(seen.h, sh=K) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cout).all())
    # the first configuration after the workspace is bound: FV_ERR_STATE; later calls with the same chunk: any time
    fresh.ensure_workspace(B, 1, False)
    assert L.fv_head_set_flow_guidance(fresh.h, K, w, 5.0) == -2 and b"fv_bind_workspace" in L.fv_last_error(fresh.h)
    assert L.fv_head_set_flow_guidance(seen.h, K, (C.c_float * K)(1.0, 0.5, 0.0), 2.0) == 0
    # set, then unset: the unguided sampler's bits, and the guided entry refuses again
    noise = torch.randn(B, da, generator=torch.Generator().manual_seed(1))
    got = [e.head_flow_sample(_flat(e, case["p"]), pooled, states, steps=4, noise=noise) for e in (fresh, seen)]
    assert L.fv_head_set_flow_guidance(seen.h, 0, None, 0.0) == 0 and call(seen.h) == -2
    got.append(seen.head_flow_sample(flat, pooled, states, steps=4, noise=noise))
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    fresh.close(), seen.close()


# ------------------------------------------------------------------------------------------------------------------ 6. surfaces
def _policy(K, n_steps, seed=0, **kw):
    from vla_fastvlm.fastvla.configuration_fastvla import FastVLAConfig
    from vla_fastvlm.fastvla.modeling_fastvla import FastVLAPolicy
    torch.manual_seed(seed)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K, n_action_steps=n_steps,
                         action_head="flow", flow_time_dim=6, flow_seed=77, **kw).to(DEV)


def _policy_reference(pol, img, st, task, call_index, prev, w, shift, guided):
    """the float64 guided reference for the policy's plan number call_index (1-based): its pooled feature, its head, its noise draw"""
    m = pol.model
    eng = m._engine()
    K, A, E = m.chunk_size, pol.config.action_dim, m.flow["time_dim"]
    with torch.no_grad():
        pooled = m.features(pol.processor.prepare_images(img.unsqueeze(0), DEV), pol.processor.prepare_tasks(task, batch_size=1), device=DEV)
        states = pol.processor.prepare_states(st.unsqueeze(0), DEV).float()
        noise = eng.head_flow_prepare(torch.zeros(1, K * A), eng.head_saved(1), seed=m._flow_seed, offset=(1 << 62) + call_index)      # u = eps - 0
    torch.cuda.synchronize()
    p = {k: v.detach().cpu().clone() for k, v in eng.head_views(m._flat).items()}
    Y, W = ru.targets(prev if guided else torch.zeros(1, K * A), w if guided else np.zeros(K), K, A, shift)
    args = (p, pooled.cpu(), states.cpu(), noise.cpu(), m.flow_steps, E, Y, W, pol.rtc["max_guidance_weight"])
    _, c64 = ru.guided_euler(*args)
    _, c32 = ru.guided_euler(*args, fp32=True)
    return c64, fu.worst_row_vs_rms(c32, c64)


def test_core_policy_replans_guided(monkeypatch):
    for k in ("FASTVLA_RTC", "FASTVLA_ACTION_HEAD", "FASTVLA_TEMPORAL_ENSEMBLE_COEFF"):
        monkeypatch.delenv(k, raising=False)
    K, n, A = 8, 3, 14
    pol, plain = _policy(K, n, rtc=True), _policy(K, n)
    assert pol.rtc["execution_horizon"] == n and plain.rtc is None
    g = torch.Generator().manual_seed(5)
    img, st, task = torch.rand(3, 72, 96, generator=g).to(DEV), torch.randn(14, generator=g).to(DEV), "open drawer"
    w = prefix_weights(K, 0, n, "exp")
    served, plans = [], []
    for i in range(3 * n):
        prev = pol.last_chunk_normalised
        served.append(pol.select_action(img, st, task, DEV))
        if i % n == 0:
            plans.append((prev, pol.last_chunk_normalised))
    assert pol.model._flow_sample_calls == 3
    # the first plan after construction is unguided: the policy without rtc serves the same bits
    first = [plain.select_action(img, st, task, DEV) for _ in range(n)]
    assert all(torch.equal(a, b) for a, b in zip(served[:n], first))
    worst = 0.0
    for j, (prev, chunk) in enumerate(plans):
        assert all(torch.equal(served[j * n + r], chunk[r]) for r in range(n))          # (no dataset statistics folded in: actions are the normalised chunk)
        c64, emu = _policy_reference(pol, img, st, task, j + 1, None if prev is None else prev.cpu().reshape(1, -1), w, n, guided=prev is not None)
        err = fu.worst_row_vs_rms(chunk.cpu().reshape(1, -1), c64)
        worst = max(worst, err / (4 * emu))
        print(f"[rtc policy plan {j}] error {err:.3e}, fp32 emulation {emu:.3e}, error / bar {err / (4 * emu):.3f}")
        assert err <= 4 * emu
    assert not torch.equal(plans[1][1], plans[0][1])
    # reset(): the next plan is unguided again
    pol.reset(), plain.reset()
    plain.model._flow_sample_calls = pol.model._flow_sample_calls
    assert torch.equal(pol.select_action(img, st, task, DEV), plain.select_action(img, st, task, DEV))
    # the explicit form: the left-over rows of the last chunk, two of them a hard prefix
    last = pol.last_chunk_normalised
    got = pol.select_action_chunk(img, st, task, DEV, prev_chunk=last[2:], inference_delay=2)
    prevbuf = torch.zeros(K, A)
    prevbuf[2:] = last[2:].cpu()
    c64, emu = _policy_reference(pol, img, st, task, pol.model._flow_sample_calls, prevbuf.reshape(1, -1), prefix_weights(K, 2, n, "exp"), 2, guided=True)
    err = fu.worst_row_vs_rms(got.cpu().reshape(1, -1), c64)
    print(f"[rtc policy explicit] error {err:.3e}, fp32 emulation {emu:.3e}, error / bar {err / (4 * emu):.3f}; hard prefix "
          f"{float((got[:2] - last[2:4]).abs().max()):.4f}")
    assert err <= 4 * emu and torch.equal(pol.last_chunk_normalised, got)
    with pytest.raises(ValueError):
        pol.select_action_chunk(img, st, task, DEV, prev_chunk=last, inference_delay=K)          # d + s > K
    with pytest.raises(ValueError, match="rtc"):
        plain.select_action_chunk(img, st, task, DEV, prev_chunk=last)
    for p_ in (pol, plain):
        p_.model.backbone.engine().close()


def test_lerobot_plugin_resets_one_environment(monkeypatch):
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    for k in ("FASTVLA_RTC", "FASTVLA_ACTION_HEAD"):
        monkeypatch.delenv(k, raising=False)
    K, A, B, n = 4, 5, 3, 2
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}

    def make(**kw):
        torch.manual_seed(3)
        cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=K, n_action_steps=n,
                       output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)
        return LRPolicy(cfg, action_head="flow", flow_time_dim=6, flow_steps=5, flow_seed=11, **kw).to(DEV)

    g = torch.Generator().manual_seed(4)
    batch = {"observation.images.top": torch.rand(B, 3, 64, 64, generator=g).to(DEV), "observation.state": torch.randn(B, 6, generator=g).to(DEV),
             "task": ["a", "b", "c"]}
    runs = []
    for reset_env in (None, 1):
        pol = make(rtc=True)
        acts = []
        for i in range(3 * n):
            if i == n and reset_env is not None:
                pol.model.rtc_reset(reset_env)                # environment 1 starts a new episode: its next plan is unguided
            acts.append(pol.select_action(batch).clone())
        assert all(a.shape == (B, A) and bool(torch.isfinite(a).all()) for a in acts) and pol.model._flow_sample_calls == 3
        runs.append(torch.stack(acts))
        if reset_env is None:
            # LeRobot's keyword set, all B environments in one call
            left = pol.last_chunk_normalised[:, 1:]
            chunk = pol.predict_action_chunk(batch, inference_delay=1, prev_chunk_left_over=left, execution_horizon=2)
            assert chunk.shape == (B, K, A) and bool(torch.isfinite(chunk).all()) and torch.equal(pol.last_chunk_normalised, chunk)
            with pytest.raises(ValueError):
                pol.predict_action_chunk(batch, inference_delay=3, prev_chunk_left_over=left, execution_horizon=2)
        pol.model.backbone.engine().close()
    same, other = runs
    assert torch.equal(same[:, [0, 2]], other[:, [0, 2]])                         # the other two environments: bit for bit
    assert torch.equal(same[:n, 1], other[:n, 1]) and not torch.equal(same[n:2 * n, 1], other[n:2 * n, 1])
    off = make()
    assert off.rtc is None and off.select_action(batch).shape == (B, A)
    with pytest.raises(ValueError, match="rtc"):
        off.predict_action_chunk(batch, inference_delay=1)
    off.model.backbone.engine().close()


def test_policy_without_rtc_keeps_the_recorded_bits(monkeypatch):
    """tools/rtc_bench.py --digest: a flow policy that does not ask for rtc serves the bits the build before real-time chunking served (the digest recorded
    in profiles/rtc_bench.json was produced by that build)"""
    import importlib.util
    import json
    from pathlib import Path
    for k in ("FASTVLA_RTC", "FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_STEPS", "FASTVLA_TEMPORAL_ENSEMBLE_COEFF"):
        monkeypatch.delenv(k, raising=False)
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("rtc_bench_tool", root / "tools" / "rtc_bench.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    want = json.loads((root / "profiles" / "rtc_bench.json").read_text())["digest"]
    assert tool.digest(torch.device(DEV)) == want
