"""-m gpu: parameter groups of the fused clip + AdamW step (fv_adamw_groups_create / fv_adamw_clip_step_groups in include/fastvla_hip.h;
csrc/optim_kernels.hip; fastvla_hip/optim.py).

The reference is restated here in float64: torch.optim.AdamW's update per group (lr_g = lr * lr_scale, the group's decay, step size lr_g / (1 - beta1^t),
denominator sqrt(v) / sqrt(1 - beta2^t) + eps) after ONE torch clip_grad_norm_ over the non-frozen elements (coef = min(max_norm / (norm + 1e-6), 1)).  The
hyper-parameters enter it as the float32 values the kernel receives.

Bounds, from the arithmetic and not from a run:
  p     |p - p64| <= 4 spacing_fp32(|p64|) + 1e-5 |p64 - p_old|, every element: the decay product and the final subtraction round to half a spacing each, the
        factor 1 - lr wd carries half an ulp of 1; the Adam term (a clip coefficient from a blocked fp32 sum over <= 5e4 terms, two divisions, a square root,
        four products) is good to a few 1e-7 of itself.
  v     relative 1e-5, every element (a sum of two non-negative products: no cancellation).
  m     NOT relative to |m| element by element, which no float32 kernel can meet: beta1 m + (1 - beta1) g cancels when the two terms have opposite signs, and
        one rounding of a term (6e-8 of it) is already 1e-5 of the result once the terms cancel 170-fold -- among 5e4 random elements dozens do.  An element
        is held to 1e-5 of the terms' magnitudes, |beta1 m_old| + |(1 - beta1) g| (the backward-error form of "relative 1e-5"), and every GROUP to 1e-5 of
        its m in relative L2.
  norms relative 1e-5, the global one and every group's.
The op-level tests apply exactly these.  The step-level tests, on a real backward's gradients, add two spacings of float32's subnormal range (2 x 2^-149) as an
absolute floor to m and v: squares of gradients below 1e-19 land under 1.2e-38, where the format itself has no relative precision.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV  # noqa: E402
from fastvla_hip import FastVLAEngine, FastVLAHipError, _lib, arch, optim  # noqa: E402

BETAS, EPS = (0.9, 0.95), 1e-8
LRS = (1e-3, 3e-3, 5e-4)          # three consecutive steps, a different lr each
F32 = lambda x: float(np.float32(x))  # noqa: E731
TINY = 2.0 * 2.0 ** -149


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    e = FastVLAEngine(arch.preset("tiny"), state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64, max_batch=2, max_text_tokens=8)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------------------ the float64 restatement
def ref_step(p, g, m, v, groups, *, lr, step, max_grad_norm, grad_scale, betas=BETAS, eps=EPS):
    """float64 tensors p, g, m, v (CPU) -> (p, m, v, global norm, group norms, the two terms of m's update); groups as build_param_groups / the tables below"""
    b1, b2, lr, eps, gs, mx = F32(betas[0]), F32(betas[1]), F32(lr), F32(eps), F32(grad_scale), F32(max_grad_norm or 0.0)
    G = g * gs
    live = torch.ones_like(G, dtype=torch.bool)
    for gr in groups:
        if gr["frozen"]:
            live[gr["begin"]: gr["end"]] = False
    norm = float(G[live].pow(2).sum().sqrt())
    coef = min(mx / (norm + F32(1e-6)), 1.0) if mx > 0 else 1.0
    G = G * coef
    bc1, bc2 = F32(1.0 - b1 ** step), F32(np.sqrt(1.0 - b2 ** step))      # the host rounds the two corrections to float32 once (launch_adamw_clip)
    P, M, V = p.clone(), m.clone(), v.clone()
    t1, t2 = b1 * m, (1.0 - b1) * G
    gnorms = []
    for gr in groups:
        s = slice(gr["begin"], gr["end"])
        if gr["frozen"]:
            gnorms.append(0.0)
            continue
        gnorms.append(float((g[s] * gs).pow(2).sum().sqrt()))
        lrg, wd = lr * F32(gr["lr_scale"]), F32(gr["weight_decay"])
        M[s] = t1[s] + t2[s]
        V[s] = b2 * v[s] + (1.0 - b2) * G[s] * G[s]
        P[s] = p[s] * (1.0 - lrg * wd) - (lrg / bc1) * M[s] / (V[s].sqrt() / bc2 + eps)
    return P, M, V, norm, gnorms, t1.abs() + t2.abs()


def check_against_ref(what, groups, old, new, ref, norm, gnorms, floor=0.0):
    """the bounds of the module docstring (floor: the absolute allowance on m and v, 0 at op level); old / new = (p, m, v) float32 CPU before / after, ref = ref_step's result"""
    P, M, V, rnorm, rgn, mterms = ref
    p_old, m_old, v_old = old
    p, m, v = new
    sp = torch.from_numpy(np.spacing(np.abs(P.numpy()).astype(np.float32)).astype(np.float64))
    bound = 4 * sp + 1e-5 * (P - p_old.double()).abs()
    ep = (p.double() - P).abs()
    worst_p = float((ep / bound).max())
    worst_v = float((((v.double() - V).abs() - floor).clamp_min(0) / V.abs().clamp_min(1e-300)).max())
    worst_m = float((((m.double() - M).abs() - floor).clamp_min(0) / mterms.clamp_min(1e-300)).max())
    worst_gm = 0.0
    for gr in groups:
        s = slice(gr["begin"], gr["end"])
        if gr["frozen"]:
            assert torch.equal(p[s], p_old[s]) and torch.equal(m[s], m_old[s]) and torch.equal(v[s], v_old[s]), f"{what}: a frozen group moved"
        else:
            worst_gm = max(worst_gm, float((m[s].double() - M[s]).norm() / M[s].norm().clamp_min(1e-300)))
    en = abs(norm - rnorm) / max(rnorm, 1e-300)
    eg = max(abs(a - b) / max(b, 1e-300) if b > 0 else abs(a) for a, b in zip(gnorms, rgn))
    print(f"[{what}] p error / bound {worst_p:.3f}; v rel {worst_v:.2e}; m / terms {worst_m:.2e}, per group rel_l2 {worst_gm:.2e}; norm rel {en:.2e}; group norms rel {eg:.2e}")
    if not bool((ep <= bound).all()):       # name the worst element before failing
        i = int((ep / bound).argmax())
        gi = next(k for k, gr in enumerate(groups) if gr["begin"] <= i < gr["end"])
        print(f"[{what}] worst element {i} in group {gi} {groups[gi]}: p_old {float(p_old[i])!r} p64 {float(P[i])!r} p {float(p[i])!r} spacing {float(sp[i]):.3e} "
              f"|dp64| {abs(float(P[i]) - float(p_old[i])):.3e} m_old {float(m_old[i])!r} m64 {float(M[i])!r} m {float(m[i])!r} |terms| {float(mterms[i]):.3e} "
              f"v_old {float(v_old[i])!r} v64 {float(V[i])!r} v {float(v[i])!r}")
    assert bool((ep <= bound).all()), f"{what}: {int((ep > bound).sum())} parameters outside 4 spacing + 1e-5 |dp|, worst {worst_p:.2f} x the bound"
    assert worst_v <= 1e-5 and worst_m <= 1e-5 and worst_gm <= 1e-5, (what, worst_v, worst_m, worst_gm)
    assert en <= 1e-5 and eg <= 1e-5, (what, en, eg)
    for gr, a in zip(groups, gnorms):
        assert not gr["frozen"] or a == 0.0


# ------------------------------------------------------------------------------------------------------------------ tables
def _table(lengths, frozen, seed):
    """consecutive groups of these lengths; distinct lr_scale in [0, 16] (0 and 16 among them), weight decay cycling through {0, 1e-2, 0.3}"""
    rng = np.random.default_rng(seed)
    k = len(lengths)
    scales = np.linspace(0.0, 16.0, k)
    scales[1:-1] += rng.uniform(-0.4, 0.4, k - 2) * (16.0 / k)       # distinct: the jitter is below half the spacing of the grid
    scales = rng.permutation(scales)
    groups, at = [], 0
    for i, n in enumerate(lengths):
        groups.append(dict(begin=at, end=at + int(n), lr_scale=float(scales[i]), weight_decay=(0.0, 1e-2, 0.3)[i % 3], frozen=i in frozen))
        at += int(n)
    assert len({g["lr_scale"] for g in groups}) == k
    return groups, at


def _tables():
    # around FV_ADAMW_SEGMENT = 8192: one float4, one short of a segment, exactly one, one over, three and a bit.  Two orders, so that every length is
    # stepped live in one and (the first and the middle group) frozen in the other.
    a = _table([4, 8188, 8192, 8196, 24584], {0, 2}, 1)
    b = _table([8196, 8192, 8188, 4, 24584], {0, 2}, 2)
    rng = np.random.default_rng(3)
    c = _table((rng.integers(1, 66, 300) * 4).tolist(), {0, 150}, 4)      # 300 groups, lengths multiples of 4 in [4, 260]
    return {"straddle": a, "straddle_reordered": b, "300_small": c}


TABLES = _tables()
CLIPS = {"clip_active": 1.0, "clip_inactive": 1e6, "clip_off": 0.0}


def _buffers(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01
    grads = [torch.randn(n, generator=g) * 3.0 for _ in LRS]
    return p, m, v, grads


def _step(eng, table, p, g, m, v, step, lr, max_grad_norm, grad_scale, n_groups, weight_decay=123.0):
    """one grouped step on device copies -> (p, m, v, norm, group norms) on the CPU (weight_decay: hp's, which the grouped entry must ignore)"""
    P, G, M, V = (t.to(DEV).contiguous() for t in (p, g, m, v))
    norm, gn = torch.full((1,), -1.0, device=DEV), torch.full((n_groups,), -1.0, device=DEV)
    eng.adamw_step(P, G, M, V, step, lr=lr, betas=BETAS, eps=EPS, weight_decay=weight_decay, max_grad_norm=max_grad_norm, grad_scale=grad_scale,
                   grad_norm_out=norm, groups=table, group_norms_out=gn)
    torch.cuda.synchronize()
    return P.cpu(), M.cpu(), V.cpu(), float(norm), gn.cpu().tolist()


@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("name", list(TABLES))
def test_grouped_step_matches_float64_adamw_per_group(eng, name, clip):
    """three consecutive steps (m / v carried over, a different lr and bias correction each) on random buffers against the float64 restatement; frozen groups
    bit-identical with norm 0 and outside the global norm; a second run of every step gives the same bits in every output"""
    groups, n = TABLES[name]
    mx, gs = CLIPS[clip], 0.25
    table = eng.adamw_groups(groups, n)
    assert table.n_groups == len(groups)
    p, m, v, grads = _buffers(n, seed=10 + len(groups))
    for step, (lr, g) in enumerate(zip(LRS, grads), start=1):
        out = _step(eng, table, p, g, m, v, step, lr, mx, gs, len(groups))
        again = _step(eng, table, p, g, m, v, step, lr, mx, gs, len(groups))
        assert all(torch.equal(a, b) for a, b in zip(out[:3], again[:3])) and out[3] == again[3] and out[4] == again[4], "two runs differ"
        ref = ref_step(p.double(), g.double(), m.double(), v.double(), groups, lr=lr, step=step, max_grad_norm=mx, grad_scale=gs)
        if clip == "clip_active":
            assert mx < ref[3]
        elif clip == "clip_inactive":
            assert mx > ref[3]
        check_against_ref(f"{name} {clip} step {step}", groups, (p, m, v), out[:3], ref, out[3], out[4])
        p, m, v = out[:3]
    table.close()


def test_unit_groups_without_clipping_equal_the_single_group_entry_bit_for_bit(eng):
    """many groups, all lr_scale 1 and hp's weight decay, clipping off: p, m, v are fv_adamw_clip_step's (the two share ONE expression, adamw_update in
    csrc/common.h); hp.weight_decay itself is ignored by the grouped entry (a wrong value is passed there)"""
    wd = 1e-2
    for name in ("straddle", "300_small"):
        groups, n = TABLES[name]
        unit = [dict(g, lr_scale=1.0, weight_decay=wd, frozen=False) for g in groups]
        table = eng.adamw_groups(unit, n)
        p, m, v, grads = _buffers(n, seed=77)
        q, mq, vq = p.clone(), m.clone(), v.clone()
        for step, (lr, g) in enumerate(zip(LRS, grads), start=1):
            for mx in (0.0, 1e9):       # no clipping at all / a clip whose coefficient is exactly 1
                out = _step(eng, table, p, g, m, v, step, lr, mx, 0.5, len(unit), weight_decay=0.77)
                P, G, M, V = (t.to(DEV).contiguous() for t in (q, g, mq, vq))
                nrm = torch.zeros(1, device=DEV)
                eng.adamw_step(P, G, M, V, step, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, max_grad_norm=mx, grad_scale=0.5, grad_norm_out=nrm)
                torch.cuda.synchronize()
                assert torch.equal(out[0], P.cpu()) and torch.equal(out[1], M.cpu()) and torch.equal(out[2], V.cpu()), (name, step, mx)
                assert abs(out[3] - float(nrm)) <= 1e-5 * float(nrm)       # (another fixed summation order)
            p, m, v = out[:3]
            q, mq, vq = P.cpu(), M.cpu(), V.cpu()
        table.close()


def test_table_and_step_argument_checks(eng):
    """every refusal of fv_adamw_groups_create is FV_ERR_ARG and names the offending group; the step refuses another n before anything is enqueued"""
    ok = [dict(begin=0, end=8, lr_scale=1.0, weight_decay=0.0, frozen=False), dict(begin=8, end=16, lr_scale=0.0, weight_decay=0.1, frozen=True)]
    eng.adamw_groups(ok, 16).close()

    def refused(groups, n, match):
        with pytest.raises(FastVLAHipError, match=match) as ei:
            eng.adamw_groups(groups, n)
        assert ei.value.status == -1

    g0, g1 = ok
    refused(ok, 0, "n = 0")
    refused(ok, -16, "n = -16")
    refused([dict(g0, end=6), dict(g1, begin=6, end=14)], 14, "n = 14")
    refused([], 16, "n_groups = 0")
    refused([dict(begin=4 * i, end=4 * i + 4, lr_scale=1.0, weight_decay=0.0, frozen=False) for i in range(65537)], 4 * 65537, "n_groups = 65537")
    refused([g0, dict(g1, begin=8, end=8)], 16, "group 1.*empty")
    refused([dict(g1, begin=8, end=16), dict(g0)], 16, "group 0")                       # unsorted
    refused([g0, dict(g1, begin=4)], 16, "group 1.*overlapping")
    refused([g0, dict(g1, begin=12)], 16, "group 1.*gap")
    refused([dict(g0, end=6), dict(g1, begin=6)], 16, "group 0.*multiples of 4")
    refused([g0, dict(g1, end=12)], 16, "group 1.*not at n")
    refused([g0, dict(g1, end=20)], 16, "group 1.*past n")
    for bad in (-1.0, float("inf"), float("nan")):
        refused([g0, dict(g1, lr_scale=bad)], 16, "group 1.*lr_scale")
        refused([dict(g0, weight_decay=bad), g1], 16, "group 0.*weight_decay")
    arr = (_lib.AdamWGroup * 2)(_lib.AdamWGroup(0, 8, 1.0, 0.0, 0, 0), _lib.AdamWGroup(8, 16, 1.0, 0.0, 0, 7))
    import ctypes as C
    out = C.c_void_p()
    assert eng.lib.fv_adamw_groups_create(eng.h, arr, 2, 16, C.byref(out)) == -1 and out.value is None
    assert b"group 1" in eng.lib.fv_last_error(eng.h) and b"reserved" in eng.lib.fv_last_error(eng.h)
    # the step: n must be the table's
    table = eng.adamw_groups(ok, 16)
    p = torch.randn(32, device=DEV)
    g, m, v = torch.randn(32, device=DEV), torch.zeros(32, device=DEV), torch.zeros(32, device=DEV)
    p0 = p.clone()
    with pytest.raises(FastVLAHipError, match="table was built for 16") as ei:
        eng.adamw_step(p, g, m, v, 1, lr=1e-3, groups=table)
    torch.cuda.synchronize()
    assert ei.value.status == -1 and torch.equal(p, p0) and float(m.abs().max()) == 0.0
    with pytest.raises(FastVLAHipError) as ei:
        eng.adamw_step(p[:16], g[:16], m[:16], v[:16], 0, lr=1e-3, groups=table)       # step is 1-based
    assert ei.value.status == -1
    table.close()
    with pytest.raises(FastVLAHipError, match="closed"):
        eng.adamw_step(p[:16], g[:16], m[:16], v[:16], 1, lr=1e-3, groups=table)
    assert _lib.FV_ADAMW_SEGMENT == 8192


# ------------------------------------------------------------------------------------------------------------------ step level: the policy's training step
def _policy(seed=41, **kw):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    torch.manual_seed(5)
    cfg = FastVLAConfig(vlm_model_name=f"synthetic:small:{seed}", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)
    pol = FastVLAPolicy(cfg).to(DEV)
    pol.train()
    un = pol.enable_backbone_training(**kw)
    return pol, un


def _batch(B=2, seed=6):
    g = torch.Generator().manual_seed(seed)
    return {"images": torch.rand(B, 3, 96, 128, generator=g).to(DEV), "states": torch.randn(B, 14, generator=g).to(DEV),
            "actions": torch.randn(B, 14, generator=g).to(DEV), "tasks": ["pick up the red cube", "open the drawer"][:B]}


def _policy_step_against_ref(what, pol, un, batch, lr, weight_decay, max_grad_norm=1.0):
    """one fused_train_step; the float64 restatement is applied to the ENGINE's own gradient buffer, so the backward's accuracy does not enter"""
    old = tuple(t.detach().cpu().clone() for t in (un.trainable, un.m, un.v))
    out = pol.fused_train_step(batch, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    torch.cuda.synchronize()
    grads = (un.lg if un.lora is not None else un.g).detach().cpu()
    groups, names = un.param_groups(weight_decay)
    assert names == un.group_names and out["group_grad_norms"].is_cuda and out["group_grad_norms"].numel() == len(groups)
    new = tuple(t.detach().cpu().clone() for t in (un.trainable, un.m, un.v))
    ref = ref_step(old[0].double(), grads.double(), old[1].double(), old[2].double(), groups, lr=lr, step=un.step_count, max_grad_norm=max_grad_norm,
                   grad_scale=1.0 / un.eng.train_loss_scale())
    assert out["group_names"] == names
    check_against_ref(what, groups, old, new, ref, float(out["grad_norm"]), out["group_grad_norms"].cpu().tolist(), floor=TINY)
    return groups, names, old, new


def test_full_finetuning_step_with_groups_matches_float64_and_leaves_the_frozen_embedding_alone():
    """One step of the `small` policy, B = 2, everything but the tower trainable, against the float64 restatement under the op-level bounds; then a second step,
    after which the frozen embedding slice of the master and of m / v still has the bits it started with.

    The second step is NOT compared with float64.  Measured once: on this batch's real gradients it puts ONE parameter at 1.04 x the p bound (element 92205, a head | projector matrix entry:
    p -5.0e-05, |dp| 1.2e-06, spacing 3.6e-12: error 2.7e-11 against 2.6e-11 allowed), and that is fp32 itself, not the kernel: m's two terms there cancel 1700-fold
    (beta1 m_old = 2.1e-05 against (1 - beta1) g, m = -2.5e-08), each term is rounded at its own magnitude (6e-13, well inside m's own bound), and lr / bc1 / denom
    = 46 carries that into p as 2.8e-11.  A bound of 4 spacings of a 5e-05 parameter has no room for it; the first step (m_old = 0: no cancellation) and the three
    consecutive steps of the op-level tests (parameters of order 1) do."""
    opts = dict(lr_scales={"decoder": 0.1, "embedding": 0.1}, no_decay=("vectors",), freeze=("embedding",), layer_decay=0.9)
    pol, un = _policy(**opts)
    assert un.optim == optim.normalize_options(**opts)
    batch = _batch()
    L = un.eng.model.llm.layers
    start = tuple(t.detach().cpu().clone() for t in (un.trainable, un.m, un.v))
    groups, names, _, _ = _policy_step_against_ref("full fine-tuning step", pol, un, batch, 1e-3, 1e-2)
    pol.fused_train_step(batch, lr=2e-3, weight_decay=1e-2)
    torch.cuda.synchronize()
    old, new = start, tuple(t.detach().cpu() for t in (un.trainable, un.m, un.v))
    assert un.step_count == 2 and not torch.equal(old[0], new[0])
    emb = next(t for t in un.tensors if t["name"] == "model.embed_tokens.weight")
    nxt = un.tensors[un.tensors.index(emb) + 1]["offset"]
    ge = next(g for g in groups if g["begin"] == emb["offset"])
    assert ge["frozen"] and ge["end"] == nxt and abs(ge["lr_scale"] - 0.1 * 0.9 ** L) < 1e-12
    for a, b in zip(old, new):
        assert torch.equal(a[emb["offset"]: nxt], b[emb["offset"]: nxt])
    assert float(un.m[emb["offset"]: nxt].abs().max()) == 0.0 and float(un.v[emb["offset"]: nxt].abs().max()) == 0.0
    by_name = dict(zip(names, groups))
    assert by_name["model.layers.0.input_layernorm.weight"]["weight_decay"] == 0.0
    assert abs(by_name["model.layers.0.self_attn.qkv_proj.weight"]["lr_scale"] - 0.1 * 0.9 ** (L - 1)) < 1e-12
    assert by_name["model.layers.0.self_attn.qkv_proj.weight"]["weight_decay"] == 1e-2
    assert float(un.g[emb["offset"]: nxt].abs().max()) > 0       # the embedding HAS a gradient: it is the table that keeps it still
    pol.model.backbone.engine().close()


@pytest.mark.parametrize("direct", [False, True])
def test_lora_step_with_lora_plus_and_undecayed_vectors(direct):
    """rank 4, LoRA+ 16, no decay on vectors, projected (with DoRA) and direct (DoRA does not run on the direct backward: plain adapters there).  A step at lr = 0
    moves no undecayed vector -- DoRA's magnitudes among them -- ... and, the decay being lr x wd, nothing else either; at lr > 0 with a zero gradient scale it is
    the decay alone that moves a matrix and leaves the magnitudes' bits alone."""
    kw = dict(lora_rank=4, lora_alpha=8.0, lora_plus_ratio=16, no_decay=("vectors",), lora_direct=direct)
    if not direct:
        kw["lora_dora"] = True
    pol, un = _policy(**kw)
    batch = _batch()
    for i, lr in enumerate((1e-3, 2e-3)):
        groups, names, old, new = _policy_step_against_ref(f"LoRA {'direct' if direct else 'projected DoRA'} step {i + 1}", pol, un, batch, lr, 0.3)
    lt = un.lora_tensors
    ga = {t["name"]: next(g for g in groups if g["begin"] <= t["offset"] < g["end"]) for t in lt}
    a0, b0 = "model.layers.0.self_attn.q_proj.lora_A.weight", "model.layers.0.self_attn.q_proj.lora_B.weight"
    assert ga[b0]["lr_scale"] == 16 * ga[a0]["lr_scale"] and ga[a0]["weight_decay"] == ga[b0]["weight_decay"] == 0.3
    vec = [t for t in lt if t["rows"] == 1]
    assert all(ga[t["name"]]["weight_decay"] == 0.0 for t in vec)
    mags = [t for t in lt if t["name"].endswith(".lora_magnitude_vector.weight")]
    assert bool(mags) == (not direct)
    # decay alone: the engine's gradient buffer zeroed and the moments cleared, one optimiser call at lr > 0 straight on the state's buffers
    un.m.zero_(); un.v.zero_()
    before = un.trainable.detach().clone()
    table = un._groups_for(0.3)
    un.eng.adamw_step(un.trainable, torch.zeros_like(un.trainable), un.m, un.v, 1, lr=1e-2, betas=BETAS, eps=EPS, weight_decay=0.3, max_grad_norm=1.0, groups=table,
                      group_norms_out=un.group_norms)
    torch.cuda.synchronize()
    sl = lambda t: slice(t["offset"], t["offset"] + t["numel"])  # noqa: E731
    for t in vec:
        assert torch.equal(un.trainable[sl(t)], before[sl(t)]), t["name"]          # magnitudes, norm weights and biases see no decay
    ta = next(t for t in lt if t["name"] == a0)
    assert not torch.equal(un.trainable[sl(ta)], before[sl(ta)])                  # a decayed matrix moves: p (1 - lr wd)
    assert torch.allclose(un.trainable[sl(ta)], before[sl(ta)] * (1 - 1e-2 * 0.3), rtol=1e-6, atol=0)
    # and at lr = 0 nothing moves at all
    before = un.trainable.detach().clone()
    un.eng.adamw_step(un.trainable, torch.ones_like(un.trainable), un.m, un.v, 2, lr=0.0, betas=BETAS, eps=EPS, weight_decay=0.3, max_grad_norm=1.0, groups=table)
    torch.cuda.synchronize()
    assert torch.equal(un.trainable, before) and float(un.m.abs().max()) > 0
    pol.model.backbone.engine().close()


def test_lora_plus_needs_lora_and_a_running_state_keeps_its_options():
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    cfg = FastVLAConfig(vlm_model_name="synthetic:small:41", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)
    pol = FastVLAPolicy(cfg).to(DEV)
    with pytest.raises(ValueError, match="lora_plus_ratio"):
        pol.enable_backbone_training(lora_plus_ratio=16)
    assert pol._unfrozen is None
    with pytest.raises(ValueError, match="unknown section"):
        pol.enable_backbone_training(lr_scales={"backbone": 0.1})
    un = pol.enable_backbone_training(no_decay=("vectors",))
    assert pol.enable_backbone_training() is un and pol.enable_backbone_training(no_decay="vectors") is un
    with pytest.raises(RuntimeError, match="already running"):
        pol.enable_backbone_training(freeze=("embedding",))
    pol.model.backbone.engine().close()


def test_no_option_keeps_the_single_group_call_and_the_checkpoint(tmp_path, monkeypatch):
    """with no option set UnfrozenState makes the old call: the grouped entry points are not reached, and optimizer.pt has no new key"""
    from vla_fastvlm.training import Trainer, TrainingConfig
    for k in ("FASTVLA_LR_SCALES", "FASTVLA_NO_DECAY", "FASTVLA_LAYER_DECAY", "FASTVLA_LORA_PLUS_RATIO", "FASTVLA_FREEZE"):
        monkeypatch.delenv(k, raising=False)
    pol, un = _policy()
    assert un.optim == {}
    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name.startswith("fv_adamw"):
                calls.append(name)
            return getattr(self._lib, name)

    un.eng.lib = Spy(un.eng.lib)
    data = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in _batch(seed=s).items()} for s in (1, 2)]
    tr = Trainer(pol, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=2, max_steps=2, num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5,
                                                 logging_steps=1000, eval_steps=1000, seed=1))
    tr.fit()
    torch.cuda.synchronize()
    assert calls == ["fv_adamw_clip_step"] * 2
    assert un.group_names is None and un.group_norms is None
    opt = torch.load(tmp_path / "a" / "checkpoints" / "step-2" / "optimizer.pt", map_location="cpu")
    assert sorted(opt) == sorted(["m", "v", "step", "global_step", "update_step", "flat", "train_backbone", "train_tower"])
    un.eng.lib = un.eng.lib._lib
    pol.model.backbone.engine().close()


def test_trainer_resume_with_options_is_bit_for_bit_and_other_options_raise(tmp_path):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    from vla_fastvlm.training import Trainer, TrainingConfig
    g = torch.Generator().manual_seed(8)

    def mk(B):
        return {"images": torch.rand(B, 3, 96, 128, generator=g), "states": torch.randn(B, 14, generator=g), "actions": torch.randn(B, 14, generator=g),
                "tasks": ["pick up the red cube", "open the drawer", "push"][:B]}

    data = [mk(2), mk(2), mk(2)]
    cfg = FastVLAConfig(vlm_model_name="synthetic:small:43", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1000, eval_steps=1000, seed=1)
    opts = dict(lora_plus_ratio=16, no_decay=("vectors",), layer_decay=0.9, lr_scales={"projector": 0.5})
    lkw = dict(lora_rank=4, lora_alpha=8.0, lora_targets=["q_proj", "v_proj", "down_proj"])

    def fresh(enable=True, **o):
        torch.manual_seed(7)
        p = FastVLAPolicy(cfg).to(DEV)
        if enable:
            p.enable_backbone_training(**lkw, **o)
        return p

    a = fresh(**opts)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=3, **tkw)).fit()
    b = fresh(**opts)
    tb = Trainer(b, data[:2], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=2, max_steps=3, **tkw))
    tb.num_training_steps = 3
    tb.fit()
    ck = tmp_path / "b" / "checkpoints" / "step-2"
    opt = torch.load(ck / "optimizer.pt", map_location="cpu")
    assert opt["optim"] == optim.normalize_options(**opts) == b._unfrozen.optim
    json.dumps(opt["optim"])                                   # plain data
    c = fresh(enable=False)                                    # the options come back with the run, as LoRA itself does
    tc = Trainer(c, data[2:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=3, resume_from=str(ck), **tkw))
    tc.num_training_steps = 3
    tc.fit()
    torch.cuda.synchronize()
    assert tc.global_step == 3 and c._unfrozen.step_count == 3 and c._unfrozen.optim == a._unfrozen.optim
    assert torch.equal(c._unfrozen.lflat, a._unfrozen.lflat) and torch.equal(c._unfrozen.m, a._unfrozen.m) and torch.equal(c._unfrozen.v, a._unfrozen.v)
    assert torch.equal(c._unfrozen.group_norms, a._unfrozen.group_norms)
    d = fresh(lora_plus_ratio=4, no_decay=("vectors",))        # a run that asks for other options does not resume
    td = Trainer(d, data[2:], None, TrainingConfig(output_dir=str(tmp_path / "d"), save_steps=1000, max_steps=3, resume_from=str(ck), **tkw))
    with pytest.raises(ValueError) as ei:
        td.fit()
    assert "'lora_plus_ratio': 16.0" in str(ei.value) and "'lora_plus_ratio': 4.0" in str(ei.value)
    e = fresh()                                                 # ... nor does one without any
    te = Trainer(e, data[2:], None, TrainingConfig(output_dir=str(tmp_path / "e"), save_steps=1000, max_steps=3, resume_from=str(ck), **tkw))
    with pytest.raises(ValueError, match="this run uses none"):
        te.fit()
    for p_ in (a, b, c, d, e):
        p_.model.backbone.engine().close()
