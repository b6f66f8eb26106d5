"""-m gpu: the guarded optimiser step (fv_step_guard / fv_adamw_clip_step_guarded in include/fastvla_hip.h; the GUARD instances of adamw_kernel /
adamw_groups_kernel and the decision kernel in csrc/optim_kernels.hip; fastvla_hip/guard.py; FastVLAPolicy.enable_step_guard).

Op level, through the C ABI on the `tiny` preset's handle, on all four forms (single group or table, EMA or not): a healthy gradient gives the unguarded
step's bits, with delta = 1 and with a gradient that carries delta = 2^-3; a poisoned gradient leaves p, m, v, e alone and halves delta; the exported state
follows tests/step_guard_util.py's reference machine exactly.  Step level: the policy's training steps in every mode compute what they computed without the
guard while nothing goes wrong, delta passes through the whole backward, a NaN batch and a saturated backward are skipped."""
import ctypes as C
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV  # noqa: E402
from step_guard_util import GuardRef, step_buffers  # noqa: E402
from fastvla_hip import FastVLAEngine, FastVLAHipError, StepGuard, _lib, arch  # noqa: E402
from fastvla_hip import guard as guard_mod  # noqa: E402

BETAS, EPS = (0.9, 0.95), 1e-8
FORMS = {"single": (False, False), "single_ema": (False, True), "table": (True, False), "table_ema": (True, True)}
# the table: 40960 floats in four groups -- one of three FV_ADAMW_SEGMENT segments, a frozen one, one with lr_scale 0, one plain segment
TABLE_N = 40960
GROUPS = [dict(begin=0, end=24576, lr_scale=1.0, weight_decay=1e-2, frozen=False), dict(begin=24576, end=28672, lr_scale=0.5, weight_decay=0.1, frozen=True),
          dict(begin=28672, end=32768, lr_scale=0.0, weight_decay=0.3, frozen=False), dict(begin=32768, end=40960, lr_scale=2.0, weight_decay=0.0, frozen=False)]
SINGLE_NS = (1027, 40004)       # 1027: the n & 3 tail; 40004: 157 blocks
ENV_KEYS = ["FASTVLA_STEP_GUARD"] + [f"FASTVLA_STEP_GUARD_{k.upper()}" for k in guard_mod.OPTION_KEYS] + ["FASTVLA_EMA_DECAY"]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    e = FastVLAEngine(arch.preset("tiny"), state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64, max_batch=2, max_text_tokens=8)
    yield e
    e.close()


def _shapes(form):
    return (TABLE_N,) if FORMS[form][0] else SINGLE_NS


def _run(eng, b, step, form, guard=None, table=None):
    """one step on device copies of b's buffers -> CPU {p, m, v, e, norm, gnorms}"""
    _, with_ema = FORMS[form]
    P, G, M, V, E = (b[k].to(DEV).clone() for k in "pgmve")
    norm = torch.full((1,), -1.0, device=DEV)
    gn = torch.full((len(GROUPS),), -1.0, device=DEV) if table is not None else None
    kw = dict(ema=E, ema_weight=0.25) if with_ema else {}
    if guard is not None:
        kw["guard"] = guard
    eng.adamw_step(P, G, M, V, step, lr=1e-3, betas=BETAS, eps=EPS, weight_decay=1e-2, max_grad_norm=1.0, grad_scale=0.25, grad_norm_out=norm, groups=table,
                   group_norms_out=gn, **kw)
    torch.cuda.synchronize()
    return dict(p=P.cpu(), m=M.cpu(), v=V.cpu(), e=E.cpu(), norm=norm.cpu(), gnorms=gn.cpu() if gn is not None else None)


def _bits_equal(a, b):
    """every tensor bitwise (NaN-safe: the comparison is on the bit patterns)"""
    for k in ("p", "m", "v", "e", "norm", "gnorms"):
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            return False
    return True


def _table(eng, form):
    return eng.adamw_groups(GROUPS, TABLE_N) if FORMS[form][0] else None


@pytest.mark.parametrize("form", list(FORMS))
def test_healthy_gradient_gives_the_unguarded_steps_bits(eng, form):
    table = _table(eng, form)
    for n in _shapes(form):
        b = step_buffers(n, seed=n % 97)
        plain = _run(eng, b, 2, form, table=table)
        assert not torch.equal(plain["p"], b["p"]) and math.isfinite(float(plain["norm"]))
        # delta = 1
        g1 = StepGuard(eng)
        out = _run(eng, b, 2, form, guard=g1, table=table)
        assert _bits_equal(out, plain), f"{form} n={n}: the guarded step at delta = 1 differs from the unguarded one"
        st = g1.state()
        assert (st["applied"], st["skipped_nonfinite"], st["skipped_saturated"], st["last_apply"], st["last_inv_delta"], st["delta_log2"]) == (1, 0, 0, 1, 1.0, 0)
        g1.close()
        # the gradient carries delta = 2^-3: the same bits as the unguarded step over the gradient that never carried it
        g2 = StepGuard(eng, init_delta_log2=-3, min_delta_log2=-12, max_delta_log2=12)
        out = _run(eng, dict(b, g=b["g"] * 0.125), 2, form, guard=g2, table=table)
        assert _bits_equal(out, plain), f"{form} n={n}: delta = 2^-3 was not divided out exactly"
        st = g2.state()
        assert (st["applied"], st["last_inv_delta"], st["delta_log2"], st["good_steps"]) == (1, 8.0, -3, 1)
        g2.close()
    if table is not None:
        table.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_poisoned_gradient_is_skipped(eng, form):
    table = _table(eng, form)
    for n in _shapes(form):
        b = step_buffers(n, seed=3 + n % 89)
        last_seg = n - 100 if table is None else GROUPS[3]["begin"] + 5      # (single group: inside the last block)
        for pos in (0, n - 1, last_seg):
            for bad in (float("nan"), float("inf"), float("-inf"), 1e20):      # 1e20 is finite: its square is not
                g = b["g"].clone()
                g[pos] = bad
                guard = StepGuard(eng, init_delta_log2=0, min_delta_log2=-4, max_delta_log2=4)
                out = _run(eng, dict(b, g=g), 2, form, guard=guard, table=table)
                what = f"{form} n={n} g[{pos}]={bad}"
                for k in "pmve":
                    assert torch.equal(out[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} moved on a skipped step"
                assert not math.isfinite(float(out["norm"])), f"{what}: the reported norm {float(out['norm'])} hides why the step was skipped"
                st = guard.state()
                assert (st["skipped_nonfinite"], st["applied"], st["last_apply"], st["delta_log2"], st["good_steps"]) == (1, 0, 0, -1, 0), (what, st)
                if table is not None:
                    assert float(out["gnorms"][1]) == 0.0 and float(out["gnorms"][2]) > 0.0
                guard.close()
    if table is not None:
        table.close()


@pytest.mark.parametrize("form", ["table", "table_ema"])
def test_nan_inside_the_frozen_group_does_not_skip(eng, form):
    table = _table(eng, form)
    b = step_buffers(TABLE_N, seed=5)
    g = b["g"].clone()
    g[GROUPS[1]["begin"]: GROUPS[1]["end"]] = float("nan")
    b = dict(b, g=g)
    plain = _run(eng, b, 3, form, table=table)
    guard = StepGuard(eng)
    out = _run(eng, b, 3, form, guard=guard, table=table)
    assert _bits_equal(out, plain) and math.isfinite(float(out["norm"])) and not torch.equal(out["p"], b["p"])
    assert guard.state()["applied"] == 1 and guard.state()["skipped_nonfinite"] == 0
    guard.close()
    table.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_scripted_run_follows_the_reference_state_machine(eng, form):
    """12 steps, growth_interval 3, growth by 2^2: flagged and poisoned steps walk delta to the floor (where a flag is applied and a poison still skips), healthy
    runs of three walk it to the ceiling, where the growth is clamped"""
    table = _table(eng, form)
    n = _shapes(form)[0]
    b = step_buffers(n, seed=7)
    poisoned = b["g"].clone()
    poisoned[n // 2] = float("inf")
    cfg = dict(init_delta_log2=0, min_delta_log2=-2, max_delta_log2=1, growth_interval=3, backoff_log2=1, growth_log2=2)
    guard = StepGuard(eng, **cfg)
    ref = GuardRef(**cfg, last_saturations=guard.state()["last_saturations"])
    assert guard.state() == ref.as_export()
    ops = _lib.load_testops()
    script = "fpfphhhhhhfh"
    deltas = []
    for step, op in enumerate(script, 1):
        if op == "f":
            _lib.check(ops.fv_op_step_guard_set_flag(guard.flag().data_ptr(), 1.0, torch.cuda.current_stream().cuda_stream), "fv_op_step_guard_set_flag")
            ref.set_flag()
            torch.cuda.synchronize()
            assert float(guard.flag()) == 1.0 and guard.state()["flag"] == 1.0       # (the flag tensor IS the guard's device word)
        out = _run(eng, dict(b, g=poisoned if op == "p" else b["g"]), step, form, guard=guard, table=table)
        applied = ref.step(float("inf") if op == "p" else 1.0)
        assert guard.state() == ref.as_export(), (form, step, op, guard.state(), ref.as_export())
        assert torch.equal(out["p"], b["p"]) == (not applied), (form, step, op)
        rep = guard.report().cpu()
        assert float(rep[0]) == float(not applied) and float(rep[1]) == math.ldexp(1.0, ref.delta_log2)
        deltas.append(ref.delta_log2)
    assert deltas == [-1, -2, -2, -2, -2, -2, 0, 0, 0, 1, 0, 0]
    assert (ref.applied, ref.skipped_nonfinite, ref.skipped_saturated, ref.saturated_applied) == (8, 2, 2, 1)
    guard.close()
    if table is not None:
        table.close()


def test_observe_sets_the_flag_when_the_saturation_counter_moved(eng):
    guard = StepGuard(eng, init_delta_log2=0, min_delta_log2=-4, max_delta_log2=4)
    guard.observe()
    torch.cuda.synchronize()
    assert guard.state()["flag"] == 0.0            # the counter stands where the guard's creation found it
    guard.close()


def test_argument_errors_launch_nothing_and_leave_the_state_alone(eng):
    n = TABLE_N
    table = eng.adamw_groups(GROUPS, n)
    other = eng.adamw_groups([dict(begin=0, end=n - 4, lr_scale=1.0, weight_decay=0.0, frozen=False)], n - 4)
    b = step_buffers(n, seed=9)
    P, G, M, V, E = (b[k].to(DEV).clone() for k in "pgmve")
    guard = StepGuard(eng, init_delta_log2=-1, min_delta_log2=-4, max_delta_log2=4)
    before = guard.state()
    hp = _lib.AdamWHParams(1e-3, 0.9, 0.95, 1e-8, 1e-2, 1.0, 1.0)

    def refused(match, ema, tab, g):
        rc = eng.lib.fv_adamw_clip_step_guarded(eng.h, P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), ema, C.c_float(0.5), n, C.byref(hp),
                                                tab.handle() if tab is not None else None, 1, g, None, None, None)
        msg = eng.lib.fv_last_error(eng.h).decode()
        assert rc == -1 and match in msg, (match, rc, msg)
        torch.cuda.synchronize()
        for k, t in zip("pgmve", (P, G, M, V, E)):
            assert torch.equal(t.cpu(), b[k]), (match, k)
        assert guard.state() == before, match

    for tab in (None, table):
        refused("guard is null", E.data_ptr(), tab, None)
        refused("ema aliases flat_params", P.data_ptr(), tab, guard.handle())
        refused("ema aliases v", V.data_ptr(), tab, guard.handle())
    refused("the table was built for", None, other, guard.handle())
    with pytest.raises(FastVLAHipError, match="init_delta_log2"):
        StepGuard(eng, init_delta_log2=3, min_delta_log2=0, max_delta_log2=2)
    with pytest.raises(FastVLAHipError, match="min_delta_log2"):
        StepGuard(eng, init_delta_log2=0, min_delta_log2=1, max_delta_log2=0)
    with pytest.raises(FastVLAHipError, match="growth_interval"):
        StepGuard(eng, growth_interval=0)
    with pytest.raises(FastVLAHipError, match="leaves \\[0, 24\\]"):      # the handle's loss scale is 2^12: 12 + 13 > 24
        StepGuard(eng, init_delta_log2=0, min_delta_log2=0, max_delta_log2=13)
    bad = dict(before, delta_log2=9)
    with pytest.raises(FastVLAHipError, match="outside the guard's"):
        guard.load_state(bad)
    assert guard.state() == before
    guard.load_state(dict(before, delta_log2=2, applied=41))
    assert guard.state() == dict(before, delta_log2=2, applied=41)
    guard.close()
    table.close()
    other.close()


# ------------------------------------------------------------------------------------------------------------------ step level: the policy's training steps
# Presets as tests/test_gpu_ema.py: head-only on `tiny`, the unfrozen modes on `small` (the smallest preset whose decoder trains).  B = 2.
MODES = {
    "head": dict(model="tiny:77", enable=None),
    "full_decoder": dict(model="small:41", enable={}),
    "lora_groups": dict(model="small:41", enable=dict(lora_rank=4, lora_alpha=8.0, lora_plus_ratio=16, no_decay=("vectors",), freeze=("projector",))),
    "lora_direct": dict(model="small:41", enable=dict(lora_rank=4, lora_alpha=8.0, lora_direct=True)),
    "tower": dict(model="small:41", enable=dict(tower=True)),
}
KW = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)


def _policy(mode, guard=None, ema=False, seed=31):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    spec = MODES[mode]
    torch.manual_seed(seed)
    cfg = FastVLAConfig(vlm_model_name=f"synthetic:{spec['model']}", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=spec["enable"] is None)
    pol = FastVLAPolicy(cfg).to(DEV)
    pol.train()
    if spec["enable"] is not None:
        pol.enable_backbone_training(**spec["enable"])
    if ema:
        pol.enable_ema(decay=0.99, warmup=False, update_after=0)
    if guard is not None:
        pol.enable_step_guard(**guard)
    return pol


def _batch(B=2, seed=6, actions=None):
    g = torch.Generator().manual_seed(seed)
    b = {"images": torch.rand(B, 3, 96, 128, generator=g).to(DEV), "states": torch.randn(B, 14, generator=g).to(DEV),
         "actions": torch.randn(B, 14, generator=g).to(DEV), "tasks": ["pick up the red cube", "open the drawer"][:B]}
    if actions is not None:
        b["actions"] = actions(b["actions"])
    return b


def _live(pol):
    un = pol._unfrozen
    return un.trainable if un is not None else pol.model._flat


def _state(pol):
    """(p, m, v) of the run, CPU copies"""
    return tuple(t.detach().cpu().clone() for t in (_live(pol), pol._opt_state["m"], pol._opt_state["v"]))


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _close(*pols):
    for p in pols:
        p.model.backbone.engine().close()


@pytest.mark.parametrize("mode", ["head", "full_decoder", "lora_groups", "lora_direct", "tower"])
def test_a_healthy_guarded_run_computes_what_the_unguarded_run_computes(mode):
    """3 updates over 4 micro-batches (one grad_accum_steps = 2 window): loss, p, m, v bitwise those of the run without the guard"""
    a, b = _policy(mode, guard=dict(growth_interval=1000)), _policy(mode)
    assert a.step_guard_enabled and not b.step_guard_enabled
    for k, seed in [(1, 11), (2, 12), (2, 13), (1, 14)]:
        batch = _batch(seed=seed)
        oa = a.fused_train_step(batch, grad_accum_steps=k, **KW)
        ob = b.fused_train_step(batch, grad_accum_steps=k, **KW)
        torch.cuda.synchronize()
        assert oa["synced"] == ob["synced"] and torch.equal(oa["loss"], ob["loss"]) and torch.equal(oa["grad_norm"], ob["grad_norm"])
        assert "step_skipped" not in ob and "loss_scale" not in ob
        assert oa["step_skipped"].is_cuda and float(oa["step_skipped"]) == 0.0
        assert float(oa["loss_scale"]) == (1.0 if mode == "head" else 4096.0)
    assert _same(_state(a), _state(b)), f"{mode}: p, m or v differs from the run without the guard"
    st = a.step_guard_stats()
    assert (st["applied"], st["skipped_nonfinite"], st["skipped_saturated"], st["saturated_applied"], st["delta_log2"], st["good_steps"]) == (3, 0, 0, 0, 0, 3)
    assert st["loss_scale_log2"] == (0 if mode == "head" else 12)
    a.disable_step_guard()
    assert "step_skipped" not in a.fused_train_step(_batch(seed=15), **KW)
    b.fused_train_step(_batch(seed=15), **KW)
    torch.cuda.synchronize()
    assert _same(_state(a), _state(b))
    _close(a, b)


@pytest.mark.parametrize("mode", ["full_decoder", "lora_direct", "tower"])
def test_delta_passes_through_the_whole_backward(mode):
    """a bound guard at delta = 2^-2 over the static 2^12 against no guard and a static 2^10: the WHOLE gradient buffer is bitwise equal -- every gradient the
    step writes carries 2^k delta, the tower's (whose stream picks a scale of its own) included"""
    a, b = _policy(mode), _policy(mode)
    ea, eb = a._unfrozen.eng, b._unfrozen.eng
    guard = StepGuard(ea, init_delta_log2=-2, min_delta_log2=-12, max_delta_log2=12)
    ea.train_set_step_guard(guard)
    eb.train_set_options(loss_scale_log2=10, keep=True)
    batch = _batch(seed=21)
    oa = a.fused_train_step(batch, **KW)
    ob = b.fused_train_step(batch, **KW)
    torch.cuda.synchronize()
    assert torch.equal(oa["loss"], ob["loss"])
    ga, gb = (p._unfrozen.lg if mode == "lora_direct" else p._unfrozen.g for p in (a, b))
    assert bool(torch.isfinite(ga).all()) and float(ga.abs().max()) > 0.0
    assert int((ga != 0).sum()) > ga.numel() // 2
    diff = int((ga.view(torch.int32) != gb.view(torch.int32)).sum())
    print(f"[step guard delta passthrough {mode}] {diff} of {ga.numel()} gradient elements differ")
    assert diff == 0, f"{mode}: {diff} gradient elements differ between 2^12 x delta 2^-2 and a static 2^10"
    with pytest.raises(FastVLAHipError, match="leaves \\[0, 24\\]"):      # while the guard is bound the static scale stays inside its range
        ea.train_set_options(loss_scale_log2=20, keep=True)
    ea.train_set_step_guard(None)
    guard.close()
    _close(a, b)


@pytest.mark.parametrize("mode", ["head", "full_decoder"])
def test_a_nan_batch_is_skipped_and_the_run_goes_on(mode):
    """delta pinned (dynamic_loss_scale=False), EMA on: the NaN batch leaves master, m, v and the shadow alone; the next healthy step is the step a guard-off run
    makes from the same state at the same step index"""
    a, b = _policy(mode, guard=dict(dynamic_loss_scale=False), ema=True), _policy(mode, ema=True)
    for pol in (a, b):
        pol.fused_train_step(_batch(seed=11), **KW)
    torch.cuda.synchronize()
    assert _same(_state(a), _state(b))
    before, shadow = _state(a), a.ema_shadow.detach().cpu().clone()

    def poison(x):
        x = x.clone()
        x[1, 3] = float("nan")
        return x
    out = a.fused_train_step(_batch(seed=12, actions=poison), **KW)
    torch.cuda.synchronize()
    assert float(out["step_skipped"]) == 1.0 and not math.isfinite(float(out["grad_norm"])) and not math.isfinite(float(out["loss"]))
    assert _same(_state(a), before), f"{mode}: a skipped step moved p, m or v"
    assert torch.equal(a.ema_shadow.cpu(), shadow), f"{mode}: a skipped step moved the EMA shadow"
    st = a.step_guard_stats()
    assert (st["applied"], st["skipped_nonfinite"], st["delta_log2"]) == (1, 1, 0)
    # the guard-off run never sees the NaN batch; its step index advances as the guarded run's did
    b._opt_state["step"] += 1
    if b._unfrozen is not None:
        b._unfrozen.step_count += 1
    oa = a.fused_train_step(_batch(seed=13), **KW)
    ob = b.fused_train_step(_batch(seed=13), **KW)
    torch.cuda.synchronize()
    assert float(oa["step_skipped"]) == 0.0 and torch.equal(oa["loss"], ob["loss"]) and a._opt_state["step"] == b._opt_state["step"] == 3
    assert _same(_state(a), _state(b)), f"{mode}: the step after a skip differs from the guard-off run's step at the same index"
    assert torch.equal(a.ema_shadow, b.ema_shadow)
    assert bool(torch.isfinite(_live(a)).all())
    _close(a, b)


def test_a_saturated_backward_is_skipped_until_the_scale_fits():
    """MSE over n = B A = 28 elements: dL/dactions = 2 (a - t) / n x 2^12.  Targets of 1e5 put it near 3e7, far outside binary16 (65504): the decoder backward's
    fp16 gradient operands clamp.  The guard skips, halves delta, and the same batch is applied at the first delta at which nothing clamps."""
    big = lambda x: x + 1e5      # noqa: E731
    batch = _batch(seed=31, actions=big)
    assert 2.0 * 1e5 / 28 * 4096 > 100 * 65504
    plain = _policy("full_decoder")
    plain.fused_train_step(batch, **KW)
    n_sat = plain._unfrozen.eng.fp16_saturations()
    print(f"[step guard saturation] the unguarded step counted {n_sat} saturated operand groups")
    assert n_sat > 0
    pol = _policy("full_decoder", guard=dict(growth_interval=1000))
    before = _state(pol)
    out = pol.fused_train_step(batch, **KW)
    torch.cuda.synchronize()
    st = pol.step_guard_stats()
    assert float(out["step_skipped"]) == 1.0 and float(out["loss_scale"]) == 2048.0
    assert (st["skipped_saturated"], st["skipped_nonfinite"], st["applied"], st["delta_log2"], st["loss_scale_log2"]) == (1, 0, 0, -1, 11)
    assert _same(_state(pol), before)
    skipped = 1
    for _ in range(12):      # 2^12 x delta reaches 1 after twelve halvings, where a flagged step is applied whatever the counter does
        out = pol.fused_train_step(batch, **KW)
        if float(out["step_skipped"]) == 0.0:
            break
        skipped += 1
        assert _same(_state(pol), before)
    st = pol.step_guard_stats()
    print(f"[step guard saturation] applied after {skipped} skipped steps at loss scale 2^{12 - skipped}: {st}")
    assert (st["applied"], st["skipped_saturated"], st["saturated_applied"], st["delta_log2"]) == (1, skipped, 0, -skipped), st
    assert not _same(_state(pol), before) and all(bool(torch.isfinite(t).all()) for t in _state(pol))
    _close(plain, pol)


@pytest.mark.parametrize("mode", ["head", "full_decoder"])
def test_trainer_checkpoint_and_resume_with_the_guard_on(mode, tmp_path):
    """3 updates, save, resume in a fresh policy, 2 more == an uninterrupted 5-update run, bitwise in p, m, v, with the guard's state restored (growth_interval 2:
    the scale has moved by the time of the checkpoint wherever there is one to move)"""
    from vla_fastvlm.training import Trainer, TrainingConfig
    gopts = dict(growth_interval=2, max_loss_scale_log2=14)
    cpu = lambda b: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()}  # noqa: E731
    data = [cpu(_batch(seed=s)) for s in (31, 32, 33, 34, 35)]
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1, eval_steps=1000, seed=1)
    a = _policy(mode, guard=gopts)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=5, **tkw)).fit()
    b = _policy(mode, guard=gopts)
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=5, **tkw))
    tb.num_training_steps = 5
    tb.fit()
    torch.cuda.synchronize()
    ck = tmp_path / "b" / "checkpoints" / "step-3"
    opt = torch.load(ck / "optimizer.pt", map_location="cpu")
    assert sorted(opt["step_guard"]) == ["options", "state"] and opt["step_guard"]["options"] == guard_mod.normalize_options(**gopts)
    rec = opt["step_guard"]["state"]
    assert rec == {k: b.step_guard_stats()[k] for k in guard_mod.STATE_KEYS}
    assert rec["applied"] + rec["skipped_nonfinite"] + rec["skipped_saturated"] == 3
    if mode == "full_decoder":
        assert rec["delta_log2"] != 0 or rec["skipped_saturated"] > 0      # two good steps grew the scale (or a grown scale saturated and came back)
    log = [json.loads(ln) for ln in (tmp_path / "b" / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert all("train/step_skipped" in r and "train/loss_scale" in r for r in log)
    c = _policy(mode, guard=gopts, seed=99 if mode == "head" else 31)
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=5, resume_from=str(ck), **tkw))
    tc.num_training_steps = 5
    tc.fit()
    torch.cuda.synchronize()
    assert tc.update_step == 5 and c._opt_state["step"] == 5
    assert _same(_state(c), _state(a)), f"{mode}: the resumed run differs from the uninterrupted one"
    sa, sc = a.step_guard_stats(), c.step_guard_stats()
    sa.pop("last_saturations"), sc.pop("last_saturations")      # (a count of the engine's own, which a fresh engine starts over)
    assert sa == sc and sa["applied"] + sa["skipped_nonfinite"] + sa["skipped_saturated"] == 5
    # other options do not resume
    d = _policy(mode, guard=dict(growth_interval=3))
    td = Trainer(d, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "d"), save_steps=1000, max_steps=5, resume_from=str(ck), **tkw))
    with pytest.raises(ValueError) as ei:
        td.fit()
    assert "'growth_interval': 2" in str(ei.value) and "'growth_interval': 3" in str(ei.value)
    _close(a, b, c, d)


def test_off_by_default_nothing_gains_a_key(tmp_path):
    from vla_fastvlm.training import Trainer, TrainingConfig
    cpu = lambda b: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()}  # noqa: E731
    pol = _policy("head")
    out = pol.fused_train_step(_batch(seed=11), **KW)
    assert "step_skipped" not in out and "loss_scale" not in out and not pol.step_guard_enabled and pol._sg is None
    Trainer(pol, [cpu(_batch(seed=s)) for s in (31, 32)], None,
            TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=2, max_steps=2, num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1,
                           eval_steps=1000, seed=1)).fit()
    ck = tmp_path / "a" / "checkpoints" / "step-2"
    opt = torch.load(ck / "optimizer.pt", map_location="cpu")
    assert "step_guard" not in opt and sorted(opt) == ["global_step", "m", "step", "update_step", "v"]
    extras = ck / "hip_extras.json"
    assert not extras.is_file() or "guard" not in extras.read_text()
    full = _policy("full_decoder")      # (an unfrozen run writes hip_extras.json)
    from vla_fastvlm.utils.checkpoint import save_policy_checkpoint
    full.fused_train_step(_batch(seed=11), **KW)
    save_policy_checkpoint(full, tmp_path / "full")
    assert (tmp_path / "full" / "hip_extras.json").is_file() and "guard" not in (tmp_path / "full" / "hip_extras.json").read_text()
    _close(full)
    log = (tmp_path / "a" / "logs" / "metrics.jsonl").read_text()
    assert "step_skipped" not in log and "loss_scale" not in log
    _close(pol)
