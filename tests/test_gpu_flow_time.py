"""-m gpu: the flow head's training-time distributions (fv_head_set_flow_time) and the loss by time bucket (fv_head_loss_per_time).

Bars.  t: one fp32 ulp at max(t_ref, 2^-24) against tests/flow_time_util.py's float64 reference rounded to fp32 -- one rounding of a double result whose own
error is far below fp32 (tests/test_flow_time_host.py holds the reference to 1e-12 of the same scale).  phi: test_gpu_flow.SINCOS_ULP ulps of the float64 sin /
cos of the fp32 argument formed from the t ACTUALLY WRITTEN.  The mean of singles: the bars of test_gpu_flow_draws' identity test (its _grad_bar, the float64
references of flow_draws_util).  The backbone route against the head-only route: 1e-3 / 1e-3 / test_gpu_train_unfrozen.GRAD_TOL, as in test_gpu_flow_draws.
Loss by bucket: counts exact; a sum within (n_b + 4) 2^-24 relative -- a fixed-order fp32 sum of n_b non-negative terms, plus the subtraction and the square.
t is read back exactly: targets 0 and noise 1 make x_t = t."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_draws_util as du  # noqa: E402
import flow_time_util as tu  # noqa: E402
import flow_util as fu  # noqa: E402
from chunk_loss_util import ragged_pad  # noqa: E402
from gpu_util import DEV, rel_l2  # noqa: E402
from test_gpu_flow import SINCOS_ULP, _engine, _flat  # noqa: E402
from test_gpu_flow_draws import _cat_rows, _draws_engine, _grad_bar  # noqa: E402
from fastvla_hip import HEAD_KEYS, _lib  # noqa: E402
from fastvla_hip.engine import flow_draw_offset  # noqa: E402

NAME = "awkward"
FEAT, DS, HID, FUS, K, A, E = fu.DIMS[NAME]
DA, XO = K * A, FEAT + HID
SEED, OFFSET = 0x1234_5678_9ABC, du.train_offset(5, 77, 2)
LOGIT = (0.3, 1.2)      # a logit-normal that is not the policy's (0, 1): the engine takes any finite pair


class Rig:
    """an engine with its saved buffer and the view of the cat rows inside it"""

    def __init__(self, B, S=1, prefix=None, eng=None, **kw):
        self.B, self.S = B, S
        self.eng = _engine(NAME, B, **kw) if eng is None else eng      # (eng: an engine configured by the caller, draws included)
        if prefix is not None:
            self.eng.set_head_flow_prefix(K, prefix, dist="uniform")
        if S != 1 and eng is None:
            self.eng.set_head_flow_draws(S)
        self.saved = self.eng.head_saved(B)
        _, self.cat = _cat_rows(self.eng, self.saved, B, S)

    def prepare(self, targets=None, offset=OFFSET, B=None, **kw):
        """-> (cat columns from x_t on, u) of one noising call, on the host"""
        if B is not None and B != self.B:
            saved = self.eng.head_saved(B)
            _, cat = _cat_rows(self.eng, saved, B, self.S)
        else:
            B, saved, cat = self.B, self.saved, self.cat
        u = self.eng.head_flow_prepare(torch.zeros(B, DA) if targets is None else targets, saved, seed=SEED, offset=offset, **kw)
        torch.cuda.synchronize()
        return cat[:, XO:].clone().cpu(), u.cpu()

    def times(self, offset=OFFSET, B=None):
        """-> (t (S B,) float32 as written, phi (S B, E)): x_t = t exactly with targets 0 and noise 1 (the LAST element: a prefix head pins none of the last step)"""
        R = self.S * (B or self.B)
        x, _ = self.prepare(offset=offset, B=B, noise=torch.ones(R, DA))
        assert bool((x[:, K * A - A:DA] == x[:, DA - 1:DA]).all())
        return x[:, DA - 1].numpy().copy(), x[:, DA:DA + E].numpy().copy()

    def close(self):
        self.eng.close()


def _check_times(rig, what, dist, a, b, lo, hi, stratify=False, offset=OFFSET):
    t, phi = rig.times(offset)
    ref = tu.draw_t_ref(rig.B, rig.S, SEED, offset, dist, a, b, lo, hi, stratify)
    err = tu.time_error(t, ref)
    lo32, hi32 = float(np.float32(lo)), float(np.float32(hi))
    assert bool((t >= np.float32(lo32)).all()) and bool((t <= np.float32(hi32)).all())
    # phi of the t actually written
    want = fu.phi_ref(t, fu.flow_freqs(E))
    ep = np.abs(phi.astype(np.float64) - want) / fu.ulp32(want)
    assert float(err.max()) <= 1.0, (what, float(err.max()), int(err.argmax()), t[err.argmax()], ref[err.argmax()])
    assert float(ep.max()) <= SINCOS_ULP, (what, float(ep.max()))
    return float(err.max()), float(ep.max()), t


# ------------------------------------------------------------------------------------------------------------------ 1. Beta times (and 4. phi)
@pytest.mark.parametrize("S", tu.DRAWS)
@pytest.mark.parametrize("B", tu.BATCHES)
def test_beta_times_match_the_float64_reference(B, S):
    rig = Rig(B, S)
    worst = worst_phi = 0.0
    for a, b in tu.BETAS:
        for lo, hi in tu.RANGES:
            rig.eng.set_head_flow_time("beta", a, b, lo, hi)
            e, ep, t = _check_times(rig, f"beta({a}, {b}) on ({lo}, {hi})", "beta", a, b, lo, hi)
            worst, worst_phi = max(worst, e), max(worst_phi, ep)
            if (a, b, lo, hi) == (1.0, 1.0, 0.0, 1.0):      # Beta(1, 1) on (0, 1) IS the uniform draw
                for s in range(S):
                    assert np.array_equal(t[s * B:(s + 1) * B], fu.draw_t_uniform(B, SEED, flow_draw_offset(OFFSET, s)))
    print(f"[flow time beta B={B} S={S}] worst |t - fl32(t_ref)| / bar {worst:.3f}; phi worst {worst_phi:.2f} ulp (bar {SINCOS_ULP})")
    rig.close()


def test_beta_times_at_the_ends_of_the_uniform():
    """a wide sweep of offsets on B = 67 rows: small and large k both occur, every (a, b) through the general inversion and the closed forms"""
    rig = Rig(67)
    worst, kmin, kmax = 0.0, 1 << 24, 0
    for i in range(6):
        off = OFFSET + 1000 * i
        k = tu.draw_k(67, SEED, off)
        kmin, kmax = min(kmin, int(k.min())), max(kmax, int(k.max()))
        for a, b in tu.BETAS + ((0.25, 0.25), (32.0, 32.0), (32.0, 0.25), (0.25, 32.0)):
            rig.eng.set_head_flow_time("beta", a, b, 0.0, 1.0)
            worst = max(worst, _check_times(rig, f"beta({a}, {b}) offset {off}", "beta", a, b, 0.0, 1.0, offset=off)[0])
    print(f"[flow time beta sweep] k from {kmin} to {kmax}; worst |t - fl32(t_ref)| / bar {worst:.3f}")
    rig.close()


# ------------------------------------------------------------------------------------------------------------------ 2. strata
@pytest.mark.parametrize("S", tu.DRAWS)
@pytest.mark.parametrize("B", tu.BATCHES)
def test_stratified_times_for_all_three_distributions(B, S):
    rig, plain = Rig(B, S), Rig(B, S)
    x_plain, u_plain = plain.prepare()                     # (targets 0: u = eps)
    g = torch.Generator().manual_seed(3 + B + S)
    t_given = torch.rand(S * B, generator=g)
    x_given, _ = plain.prepare(t=t_given)
    worst = 0.0
    for dist, a, b, lo, hi in (("uniform", 0.0, 1.0, 0.0, 1.0), ("uniform", 0.0, 1.0, 0.001, 1.0), ("logit_normal", *LOGIT, 0.0, 1.0),
                               ("logit_normal", 0.0, 1.0, 0.001, 1.0), ("beta", 1.5, 1.0, 0.001, 1.0), ("beta", 2.0, 5.0, 0.0, 1.0), ("beta", 0.25, 4.0, 0.0, 1.0)):
        rig.eng.set_head_flow_time(dist, a, b, lo, hi, stratify=True)
        if S == 1 and dist == "logit_normal":
            # one draw: no strata, and the logit-normal keeps its Box-Muller form and bits (the range is applied to them in double, rounded once)
            t, _ = rig.times()
            tau32 = _LogitRig.get(B, a, b).times()[0]
            assert np.array_equal(t, tu.scale_ref(tau32.astype(np.float64), lo, hi).astype(np.float32))
        else:
            e, _, t = _check_times(rig, f"stratified {dist}({a}, {b}) on ({lo}, {hi})", dist, a, b, lo, hi, stratify=True)
            worst = max(worst, e)
            if S > 1 and (lo, hi) == (0.0, 1.0) and dist == "uniform":      # draw s lies in stratum s
                for s in range(S):
                    ts = t[s * B:(s + 1) * B].astype(np.float64)
                    assert bool((ts >= np.float32(s / S) - 1e-7).all()) and bool((ts <= np.float32((s + 1) / S) + 1e-7).all())
        # eps and u are the plain head's bits under every setting; an explicit t wins over every setting
        x, u = rig.prepare()
        assert torch.equal(u, u_plain)
        xg, ug = rig.prepare(t=t_given)
        assert torch.equal(xg, x_given) and torch.equal(ug, u_plain)
    print(f"[flow time strata B={B} S={S}] worst |t - fl32(t_ref)| / bar {worst:.3f}")
    _LogitRig.close()
    rig.close(), plain.close()


class _LogitRig:
    """the plain logit-normal head (set_head_flow's own), for the one-draw comparisons"""
    rigs = {}

    @classmethod
    def get(cls, B, a, b):
        key = (B, a, b)
        if key not in cls.rigs:
            eng = _engine(NAME, B, flow=False)
            eng.set_head_flow(E, time_dist="logit_normal", dist_a=a, dist_b=b)
            cls.rigs[key] = Rig(B, 1, eng=eng)
        return cls.rigs[key]

    @classmethod
    def close(cls):
        for r in cls.rigs.values():
            r.close()
        cls.rigs = {}


# ------------------------------------------------------------------------------------------------------------------ 3. rows and draws stay independent
@pytest.mark.parametrize("stratify", [False, True])
def test_rows_and_draws_stay_independent(stratify):
    S = 3
    rig, one = Rig(67, S), Rig(67, 1)
    for r in (rig, one):
        r.eng.set_head_flow_time("beta", 2.0, 5.0, 0.001, 1.0, stratify=stratify)
    x67, u67 = rig.prepare()
    x3, u3 = rig.prepare(B=3)
    for s in range(S):
        # rows 0 .. 2 of every draw of the B = 67 call are the B = 3 call's rows, bit for bit
        assert torch.equal(x3[s * 3:(s + 1) * 3], x67[s * 67:s * 67 + 3]) and torch.equal(u3[s * 3:(s + 1) * 3], u67[s * 67:s * 67 + 3])
        x1, u1 = one.prepare(offset=flow_draw_offset(OFFSET, s))
        assert torch.equal(u1, u67[s * 67:(s + 1) * 67])                                     # eps never moves
        same_t = torch.equal(x1, x67[s * 67:(s + 1) * 67])
        # without strata draw s IS the single-draw call at offset + (s << 56); with strata only draw 0's NOISE is, its t lies in the first third
        assert same_t if not stratify else not same_t
    rig.close(), one.close()


# ------------------------------------------------------------------------------------------------------------------ 5. the prefix head
def test_prefix_head_draws_the_same_delays_under_a_beta_time():
    B, S, D = 67, 3, 2
    uni, beta = Rig(B, S, prefix=D), Rig(B, S, prefix=D)
    beta.eng.set_head_flow_time("beta", 1.5, 1.0, 0.001, 1.0, stratify=True)
    g = torch.Generator().manual_seed(1)
    targets = torch.randn(B, DA, generator=g)
    xu, uu = uni.prepare(targets)
    xb, ub = beta.prepare(targets)
    mask_u, mask_b = xu[:, DA + E:], xb[:, DA + E:]
    assert mask_u.shape[1] == K and torch.equal(mask_u, mask_b) and torch.equal(uu, ub)      # the delays (word z) and eps are the uniform head's bits
    delays = mask_u.sum(1)
    assert set(delays.tolist()) == {0.0, 1.0, 2.0} and not torch.equal(xu[:, DA:DA + E], xb[:, DA:DA + E])
    # the pinned steps are copies of the targets under either time, and the PREFIX instance's t is the reference's
    for r in range(S * B):
        pin = int(delays[r]) * A
        assert torch.equal(xb[r, :pin], targets[r % B, :pin]) and torch.equal(xu[r, :pin], targets[r % B, :pin])
    e, _, _ = _check_times(beta, "prefix head, stratified pi0", "beta", 1.5, 1.0, 0.001, 1.0, stratify=True)
    print(f"[flow time prefix] worst |t - fl32(t_ref)| / bar {e:.3f}; delays drawn: {sorted(set(delays.tolist()))}")
    uni.close(), beta.close()


# ------------------------------------------------------------------------------------------------------------------ 6. off means off
@pytest.mark.parametrize("time_dist", ["uniform", "logit_normal"])
def test_off_means_off_and_the_setter_checks(time_dist):
    B, S = 9, 3
    fresh, seen = Rig(B, S, time_dist=time_dist), Rig(B, S, time_dist=time_dist)
    L = seen.eng.lib
    g = torch.Generator().manual_seed(2)
    targets = torch.randn(B, DA, generator=g)
    want = fresh.prepare(targets)
    seen.eng.set_head_flow_time("beta", 2.0, 5.0, 0.001, 1.0, stratify=True)
    got = seen.prepare(targets)
    assert torch.equal(got[1], want[1]) and not torch.equal(got[0], want[0]) and seen.eng.head_flow_time["dist"] == "beta"
    # every bad spec: its code, nothing changed
    Spec = _lib.HeadFlowTimeSpec
    nan, inf = float("nan"), float("inf")
    for bad in (Spec(3, 1, 1, 0, 1, 0), Spec(-1, 1, 1, 0, 1, 0), Spec(2, 0.2, 1, 0, 1, 0), Spec(2, 1, 32.5, 0, 1, 0), Spec(2, nan, 1, 0, 1, 0), Spec(1, 0, inf, 0, 1, 0),
                Spec(0, 0, 1, nan, 1, 0), Spec(0, 0, 1, 0, inf, 0), Spec(0, 0, 1, 0.5, 0.5, 0), Spec(0, 0, 1, 0.6, 0.4, 0), Spec(0, 0, 1, -0.1, 1, 0), Spec(0, 0, 1, 0, 1.1, 0),
                Spec(0, 0, 1, 0, 1, 2), Spec(0, 0, 1, 0, 1, -1)):
        assert L.fv_head_set_flow_time(seen.eng.h, C.byref(bad)) == -1 and b"fv_head_set_flow_time" in L.fv_last_error(seen.eng.h)
    assert L.fv_head_set_flow_time(None, None) == -1
    reg = _engine(NAME, B, flow=False)
    ok = Spec(2, 1.5, 1.0, 0.001, 1.0, 0)
    assert L.fv_head_set_flow_time(reg.h, C.byref(ok)) == -2 and L.fv_head_set_flow_time(reg.h, None) == -2      # the regression head draws no time
    with pytest.raises(ValueError):
        seen.eng.set_head_flow_time("beta", 0.1, 1.0)
    again = seen.prepare(targets)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    # fv_head_set_flow's own time_dist = 2 stays refused
    spec2 = _lib.HeadFlowSpec(E, 4e-3, 4.0, 2, 0.0, 1.0)
    assert L.fv_head_set_flow(reg.h, C.byref(spec2)) == -1
    # set, then NULL: x_t, phi and u of a fresh handle, bit for bit
    seen.eng.set_head_flow_time(None)
    off = seen.prepare(targets)
    assert seen.eng.head_flow_time is None and torch.equal(off[0], want[0]) and torch.equal(off[1], want[1])
    # a setting that amounts to the handle's own distribution on [0, 1] gives its bits too (the plain instances run)
    a, b = (0.0, 1.0)
    seen.eng.set_head_flow_time(time_dist, a, b, 0.0, 1.0)
    same = seen.prepare(targets)
    assert torch.equal(same[0], want[0]) and torch.equal(same[1], want[1])
    # fv_head_set_flow(NULL), and a fresh fv_head_set_flow(spec), clear it (both are configuration calls of a handle that has run nothing yet)
    for how in ("null", "spec"):
        eng = _engine(NAME, B, time_dist=time_dist)
        eng.set_head_flow_time("beta", 2.0, 5.0, 0.001, 1.0)
        if how == "null":
            eng.set_head_flow(None)
        eng.set_head_flow(E, time_dist=time_dist)
        assert eng.head_flow_time is None
        eng.set_head_flow_draws(S)
        reset = Rig(B, S, eng=eng)
        cleared = reset.prepare(targets)
        assert torch.equal(cleared[0], want[0]) and torch.equal(cleared[1], want[1])
        reset.close()
    fresh.close(), seen.close(), reg.close()


# ------------------------------------------------------------------------------------------------------------------ 7. the mean of singles under strata
@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("B", du.BATCHES)
def test_stratified_step_is_the_mean_of_single_draw_steps_at_its_own_times(B, kind):
    """A stratified S = 3 step at offset o against the mean of three single-draw steps at o + (s << 56) that are handed the device's own t rows as explicit
    buffers (their eps is then the S-draw step's, bit for bit), both against the float64 reference on the noise the device drew: test_gpu_flow_draws' identity
    test with its bars, the strata being the one thing that differs."""
    S = 3
    c = du.case(NAME, B, S, seed=1)
    seed, o = 991, du.train_offset(3, 1000, 1)
    pad = ragged_pad(B, K, seed=2) if B * K > 1 else None
    eng, one = _draws_engine(NAME, B, S), _draws_engine(NAME, B, 1)
    eng.set_head_flow_time("beta", 1.5, 1.0, 0.001, 1.0, stratify=True)
    for e in (eng, one):
        e.set_head_loss(kind, 1.0, K)
    flat = _flat(eng, c["p"])
    pooled, states = c["pooled"].to(DEV), c["states"].to(DEV)
    saved = eng.head_saved(B)
    _, cat = _cat_rows(eng, saved, B, S)
    eps = eng.head_flow_prepare(torch.zeros(B, DA), saved, seed=seed, offset=o).cpu()
    eng.head_flow_prepare(torch.zeros(B, DA), saved, seed=seed, offset=o, noise=torch.ones(S * B, DA))
    torch.cuda.synchronize()
    t = cat[:, XO].clone().cpu()
    assert float(tu.time_error(t.numpy(), tu.draw_t_ref(B, S, seed, o, "beta", 1.5, 1.0, 0.001, 1.0, True)).max()) <= 1.0

    def step(e, off_, t_rows=None):
        sv = e.head_saved(B)
        u = e.head_flow_prepare(c["a"], sv, seed=seed, offset=off_, t=t_rows)
        v, _ = e.head_forward(flat, pooled, states, saved=sv, normalized_actions=True)
        loss, grads = e.head_backward(flat, v, u, sv, pad=pad)
        torch.cuda.synchronize()
        return float(loss), grads.clone(), v.clone()

    lm, gm, vm = step(eng, o)
    singles = [step(one, flow_draw_offset(o, s), t[s * B:(s + 1) * B]) for s in range(S)]
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
    print(f"[flow time identity B={B} {kind}] loss stratified {lm:.6f} mean of singles {ls:.6f} float64 {rl:.6f}; worst error / bar {worst:.3f}")
    eng.close(), one.close()


def test_backbone_route_draws_the_stratified_times_of_the_head_only_route():
    """`small`, full fine-tuning, S = 3, stratified pi0 time: the route's own noising launch against the head-only route on an inference forward's pooled
    feature and the same (seed, offset) -- the bars of test_gpu_flow_draws' route test"""
    from oracle import fastvit_hd
    from fastvla_hip import arch
    from test_gpu_flow_draws import ROUTE, _route_rig
    from test_gpu_train_unfrozen import GRAD_TOL, _inputs
    r, S = ROUTE, 3
    model = arch.preset("small")
    B, T, Kr, da = r["B"], r["T"], r["K"], r["K"] * r["A"]
    w, eng, flat = _route_rig(model, 41, r["hd"], B, T, da, r["E"], S)
    eng.set_head_flow_time("beta", 1.5, 1.0, 0.001, 1.0, stratify=True)      # (allowed at any time: no size depends on it)
    tower_out, ids, mask, states, _ = _inputs(model, B, T, 42)
    targets = torch.randn(B, da, generator=torch.Generator().manual_seed(43))
    eng.set_head_loss("mse", 1.0, Kr)
    ws = eng.train_workspace(B, T)
    scale = eng.train_loss_scale()
    o = r["offset"]

    def head_only():
        with torch.no_grad():
            tok = fastvit_hd.projector_forward(w, tower_out.float()).to(DEV)
        pooled = eng.llm_pooled(ids, mask.sum(1), tok)
        hflat = flat[: eng.head_numel()].clone()
        saved = eng.head_saved(B)
        u = eng.head_flow_prepare(targets, saved, seed=r["seed"], offset=o)
        v, _ = eng.head_forward(hflat, pooled, states.to(DEV), saved=saved, normalized_actions=True)
        loss, grads = eng.head_backward(hflat, v, u, saved)
        torch.cuda.synchronize()
        return v[:B].clone(), float(loss), grads.clone()

    rv, rl, rg = head_only()
    a, l, g = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, seed=r["seed"], offset=o,
                                         flat_grads=torch.zeros_like(flat))
    torch.cuda.synchronize()
    v, loss, g = a.clone(), float(l), g / scale
    views = lambda x: {k: t.clone() for k, t in eng.head_views(x[: eng.head_numel()]).items()}  # noqa: E731
    got, want = views(g), views(rg)
    errs = sorted(((rel_l2(got[k].cpu(), want[k].cpu()), k) for k in HEAD_KEYS), reverse=True)
    ra, el = rel_l2(v.cpu(), rv.cpu()), abs(loss - rl) / rl
    print(f"[flow time route full S={S} vs head-only] velocity rel_l2 {ra:.2e} loss rel {el:.2e}; worst head gradients: " + "; ".join(f"{k} {e:.2e}" for e, k in errs[:3]))
    assert ra <= 1e-3 and el <= 1e-3 and all(e <= GRAD_TOL for e, _ in errs), errs[:3]
    # the setting matters on this route: without it the same step gives another loss
    eng.set_head_flow_time(None)
    _, l0, _ = eng.train_forward_backward(flat, tower_out.to(DEV), ids, mask.sum(1), states, targets, ws, training=False, seed=r["seed"], offset=o,
                                          flat_grads=torch.zeros_like(flat))
    torch.cuda.synchronize()
    assert float(l0) != loss
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 8. the loss by time bucket
@pytest.fixture(scope="module")
def bucket_engines():
    engines = {}
    yield lambda B: engines.setdefault(B, _engine(NAME, B))
    for e in engines.values():
        e.close()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nb", [1, 10, 64])
@pytest.mark.parametrize("B", tu.BATCHES)
def test_loss_per_time_matches_float64(B, nb, masked, bucket_engines):
    eng = bucket_engines(B)
    eng.set_head_loss("l1", 1.0, K)      # (the kind is ignored: the metric is the squared error)
    g = torch.Generator().manual_seed(7 + B + nb)
    v, u, t = torch.randn(B, DA, generator=g), torch.randn(B, DA, generator=g), torch.rand(B, generator=g)
    t[0] = 1.0                                              # lands in the last bucket
    if B > 1:
        t[1] = 0.0
    if B > 2:
        t[2] = (1.0 / nb) if nb > 1 else 0.5               # a bucket's lower edge belongs to it
    pad = ragged_pad(B, K, seed=4) if masked else None
    if masked and B > 1:
        pad[0] = True                                       # a row without a valid step
    out = eng.head_loss_per_time(v, u, t, nb, pad=pad)
    out2 = eng.head_loss_per_time(v, u, t, nb, pad=pad)
    torch.cuda.synchronize()
    assert out.shape == (nb, 2) and torch.equal(out, out2)
    sums, counts = tu.loss_per_time_ref(v.numpy(), u.numpy(), t.numpy(), nb, pad, B, K)
    got = out.cpu().double().numpy()
    assert np.array_equal(got[:, 1], counts.astype(np.float64))
    rel = np.abs(got[:, 0] - sums) / np.maximum(sums, 1e-300) / ((counts + 4) * 2.0 ** -24)
    rel[counts == 0] = 0.0
    assert bool((got[counts == 0] == 0.0).all())            # an empty bucket reads (0, 0)
    print(f"[loss per time B={B} buckets={nb} masked={masked}] {int((counts > 0).sum())} buckets hold rows; worst sum error / bar {float(rel.max()):.3f}")
    assert float(rel.max()) <= 1.0
    if not masked:
        assert counts[nb - 1] >= DA and counts.sum() == B * DA      # t = 1.0 is in the last bucket, every element is counted once


def test_loss_per_time_with_draws_and_its_refusals():
    B, S, nb = 9, 3, 10
    eng = _draws_engine(NAME, B, S)
    eng.set_head_loss("mse", 1.0, K)
    g = torch.Generator().manual_seed(11)
    v, u, t = torch.randn(S * B, DA, generator=g), torch.randn(S * B, DA, generator=g), torch.rand(S * B, generator=g)
    pad = ragged_pad(B, K, seed=5)
    out = eng.head_loss_per_time(v, u, t, nb, pad=pad)      # the draws share their observation's mask
    torch.cuda.synchronize()
    sums, counts = tu.loss_per_time_ref(v.numpy(), u.numpy(), t.numpy(), nb, pad, B, K)
    got = out.cpu().double().numpy()
    assert np.array_equal(got[:, 1], counts.astype(np.float64))
    assert bool((np.abs(got[:, 0] - sums) <= (counts + 4) * 2.0 ** -24 * sums).all())
    # refused with nothing enqueued
    L = eng.lib
    dv, du_, dt = v.to(DEV), u.to(DEV), t.to(DEV)
    canary = torch.full((64, 2), float("nan"), device=DEV)
    args = lambda **k: [k.get("h", eng.h), k.get("a", dv.data_ptr()), k.get("u", du_.data_ptr()), k.get("t", dt.data_ptr()), k.get("B", B), k.get("nb", nb),  # noqa: E731
                        k.get("out", canary.data_ptr()), None]
    for kw in (dict(a=None), dict(u=None), dict(t=None), dict(out=None), dict(B=0), dict(B=-3), dict(nb=0), dict(nb=65), dict(h=None)):
        assert L.fv_head_loss_per_time(*args(**kw)) == -1, kw
    reg = _engine(NAME, B, flow=False)
    assert L.fv_head_loss_per_time(*args(h=reg.h)) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(canary).all())
    with pytest.raises(ValueError):
        eng.head_loss_per_time(v, u, t, 0)
    eng.close(), reg.close()


# ------------------------------------------------------------------------------------------------------------------ 9. the policy level
def _policy(Kc=3, seed=31, **kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    torch.manual_seed(seed)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:small:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=Kc, n_action_steps=1,
                         action_head="flow", flow_time_dim=6, flow_seed=77, **kw).to(DEV)


TIME_ENV = ("FASTVLA_ACTION_HEAD", "FASTVLA_EMA_DECAY", "FASTVLA_FLOW_NOISE_DRAWS", "FASTVLA_FLOW_TIME_DIST", "FASTVLA_FLOW_TIME_RANGE", "FASTVLA_FLOW_TIME_STRATIFY")


def test_policy_trains_with_the_pi0_time_resumes_and_measures_the_loss_by_time(tmp_path, monkeypatch):
    """`small`, head-only, K = 3, flow_time_dist="pi0": three updates, save, resume in a fresh policy built from the same options, the fourth update == an
    uninterrupted four-update run bit for bit in p, m, v; the record round-trips through a checkpoint; flow_loss_per_time repeats its bits and leaves the next
    training step's bits alone."""
    import json
    from test_gpu_flow import _batch, _dev
    from vla_fastvlm.training import Trainer, TrainingConfig
    from vla_fastvlm.utils import load_policy_from_checkpoint
    for k in TIME_ENV:
        monkeypatch.delenv(k, raising=False)
    Kc, B = 3, 4
    data = [_batch(B, Kc, s) for s in (31, 32, 33, 34)]
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1, eval_steps=1000, seed=1)
    a = _policy(Kc, flow_time_dist="pi0")
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=4, **tkw)).fit()
    b = _policy(Kc, flow_time_dist="pi0")
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=4, **tkw))
    tb.num_training_steps = 4
    tb.fit()
    ck = tmp_path / "b" / "checkpoints" / "step-3"
    rec = json.loads((ck / "hip_extras.json").read_text())["action_head"]
    assert rec["time_dist"] == "beta:1.5,1.0" and rec["time_range"] == [0.001, 1.0] and "time_stratify" not in rec and (rec["dist_a"], rec["dist_b"]) == (0.0, 1.0)
    c = _policy(Kc, seed=99, flow_time_dist="pi0")
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=4, resume_from=str(ck), **tkw))
    tc.num_training_steps = 4
    tc.fit()
    torch.cuda.synchronize()
    assert c._opt_state["step"] == 4 and c.model._engine().head_flow_time["dist"] == "beta"
    assert torch.equal(c.model._flat, a.model._flat) and torch.equal(c._opt_state["m"], a._opt_state["m"]) and torch.equal(c._opt_state["v"], a._opt_state["v"])
    # the time distribution matters: the same four updates with the uniform time end elsewhere
    d = _policy(Kc)
    Trainer(d, data, None, TrainingConfig(output_dir=str(tmp_path / "d"), save_steps=1000, max_steps=4, **tkw)).fit()
    assert not torch.equal(d.model._flat, a.model._flat) and d.model._engine().head_flow_time is None
    # a loaded checkpoint is a pi0 policy again
    back = load_policy_from_checkpoint(str(ck), DEV).to(DEV)
    assert back.model.flow_time == b.model.flow_time and back.model.flow_record()["time_dist"] == "beta:1.5,1.0"
    # flow_loss_per_time: every bucket is covered, two calls agree bit for bit, no counter advances, and the next training step is not disturbed
    batch = _dev(_batch(B, Kc, 5))
    counters = lambda p_: (p_.model._flow_loss_calls, p_.model._flow_eval_index, p_.model._flow_sample_calls, p_.model._drop_calls)  # noqa: E731
    before = counters(a)
    m1, n1 = a.flow_loss_per_time(batch, buckets=4)
    m2, n2 = a.flow_loss_per_time(batch, buckets=4)
    torch.cuda.synchronize()
    assert m1.shape == (4,) and n1.shape == (4,) and m1.device.type == "cuda" and torch.equal(m1, m2) and torch.equal(n1, n2) and counters(a) == before
    valid = int((~batch["action_is_pad"]).sum()) * 14
    assert float(n1.sum()) == valid and bool((n1 > 0).all()) and bool((m1 > 0).all()) and bool(torch.isfinite(m1).all())
    m10, n10 = a.flow_loss_per_time(batch)                   # 10 buckets over 4 rows: six are empty and read 0
    assert m10.shape == (10,) and int((n10 > 0).sum()) == 4 and bool((m10[n10 == 0] == 0).all())
    a.train(), c.train()
    oa, oc = a.fused_train_step(batch, lr=1e-3), c.fused_train_step(batch, lr=1e-3)      # (c never called the metric)
    torch.cuda.synchronize()
    assert torch.equal(oa["loss"], oc["loss"]) and torch.equal(a.model._flat, c.model._flat)
    for p_ in (a, b, c, d, back):
        p_.model.backbone.engine().close()
