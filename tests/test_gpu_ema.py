"""-m gpu: the EMA of the trainable weights kept by the fused clip + AdamW step (fv_adamw_clip_step_ema in include/fastvla_hip.h; the EMA instances of
adamw_kernel / adamw_groups_kernel; fastvla_hip/ema.py; FastVLAPolicy.enable_ema / ema_weights / apply_ema).

Op level, through the C ABI on the `tiny` preset's handle: p, m, v and the norms of the EMA step are BITWISE those of the step without it; the average obeys
the bound of tests/ema_util.py (derived: two roundings, doubled), copies p_new at w = 1, keeps its bits at w = 0 and in a frozen group, and has e = p as a
fixed point.  Step level: the policy's training steps in every mode keep the average on synced micro-batches only and compute what they computed without it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ema_util import check_ema  # noqa: E402
from gpu_util import DEV  # noqa: E402
from fastvla_hip import FastVLAEngine, FastVLAHipError, _lib, arch  # noqa: E402
from fastvla_hip import ema as ema_mod  # noqa: E402

BETAS, EPS = (0.9, 0.95), 1e-8
F32 = lambda x: float(np.float32(x))  # noqa: E731
WEIGHTS = {"one": 1.0, "zero": 0.0, "decay_0.999": F32(1.0 - 0.999), "nine_elevenths": F32(9.0 / 11.0)}
# 4 | a full segment and a 3-float4 tail | two full segments | 260 (frozen) | 1028: one float4 past the block's 256
LENGTHS, FROZEN = (4, 8192 + 12, 2 * 8192, 260, 1028), 3


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    e = FastVLAEngine(arch.preset("tiny"), state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64, max_batch=2, max_text_tokens=8)
    yield e
    e.close()


def _groups():
    groups, at = [], 0
    for i, n in enumerate(LENGTHS):
        groups.append(dict(begin=at, end=at + n, lr_scale=(1.0, 0.25, 2.0, 0.5, 4.0)[i], weight_decay=(0.0, 1e-2, 0.3, 0.1, 0.05)[i], frozen=i == FROZEN))
        at += n
    return groups, at


def _buffers(n, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g) * 3.0, m=torch.randn(n, generator=g) * 0.1, v=torch.rand(n, generator=g) * 0.01,
                e=torch.randn(n, generator=g))


def _dev(t, offset):
    """a device copy whose first element sits `offset` floats behind a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 4, device=DEV)
    view = buf[offset: offset + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * offset
    return view


def _run(eng, b, step, *, w=None, table=None, n_groups=0, offset=0, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, grad_scale=0.25, e=None):
    """one step on device copies of b's p, g, m, v (and, with w, the average e) -> CPU {p, m, v, e, norm, gnorms}"""
    P, G, M, V = (_dev(b[k], offset) for k in "pgmv")
    E = _dev(b["e"] if e is None else e, offset) if w is not None else None
    norm = torch.full((1,), -1.0, device=DEV)
    gn = torch.full((n_groups,), -1.0, device=DEV) if table is not None else None
    kw = dict(ema=E, ema_weight=w) if w is not None else {}
    eng.adamw_step(P, G, M, V, step, lr=lr, betas=BETAS, eps=EPS, weight_decay=weight_decay, max_grad_norm=max_grad_norm, grad_scale=grad_scale, grad_norm_out=norm,
                   groups=table, group_norms_out=gn, **kw)
    torch.cuda.synchronize()
    return dict(p=P.cpu().clone(), m=M.cpu().clone(), v=V.cpu().clone(), e=E.cpu().clone() if E is not None else None, norm=float(norm),
                gnorms=gn.cpu().tolist() if gn is not None else None)


def _same_step(a, b):
    return all(torch.equal(a[k], b[k]) for k in "pmv") and a["norm"] == b["norm"] and a["gnorms"] == b["gnorms"]


def _five_assertions(what, eng, b, w, live, still_table=None, **kw):
    """the five assertions for one weight; live: bool mask of the elements the step may touch; still_table: the table of the same groups without decay"""
    plain = _run(eng, b, 2, **kw)
    out = _run(eng, b, 2, w=w, **kw)
    assert _same_step(plain, out), f"{what}: p, m, v or a norm differs from the step without EMA"            # 1
    assert torch.equal(out["e"][~live], b["e"][~live]), f"{what}: a frozen group's average moved"              # 2
    assert not torch.equal(out["p"][live], b["p"][live])
    check_ema(what, out["e"][live], b["e"][live], out["p"][live], w)                                          # 3 (w = 1, w = 0 bitwise) and 5
    # 4: e == p is a fixed point -- a second step that cannot move p (zero gradient, lr = 0, no decay) on a buffer whose average equals its parameters
    still = dict(b, p=out["p"], m=out["m"], v=out["v"], g=torch.zeros_like(b["g"]), e=out["p"])
    kw2 = dict(kw, table=still_table) if still_table is not None else kw
    again = _run(eng, still, 3, w=w, lr=0.0, weight_decay=0.0, **kw2)
    assert torch.equal(again["p"], out["p"]) and torch.equal(again["e"], again["p"]), f"{what}: e = p is not a fixed point of the update"


@pytest.mark.parametrize("wname", list(WEIGHTS))
def test_grouped_ema_step(eng, wname):
    groups, n = _groups()
    table = eng.adamw_groups(groups, n)
    zero = eng.adamw_groups([dict(g, weight_decay=0.0) for g in groups], n)
    b = _buffers(n, seed=21)
    live = torch.ones(n, dtype=torch.bool)
    live[groups[FROZEN]["begin"]: groups[FROZEN]["end"]] = False
    plain = _run(eng, b, 2, table=table, n_groups=len(groups))
    assert plain["gnorms"][FROZEN] == 0.0 and all(x > 0 for i, x in enumerate(plain["gnorms"]) if i != FROZEN)
    _five_assertions(f"grouped {wname}", eng, b, WEIGHTS[wname], live, still_table=zero, table=table, n_groups=len(groups))
    table.close()
    zero.close()


@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("n,offset", [(1, 0), (4099, 0), (4099, 1)])
def test_single_group_ema_step(eng, n, offset, wname):
    b = _buffers(n, seed=22 + n)
    _five_assertions(f"single n={n} offset={offset} {wname}", eng, b, WEIGHTS[wname], torch.ones(n, dtype=torch.bool), offset=offset)


def test_one_unit_group_gives_the_single_group_average_bit_for_bit(eng):
    """the property adamw_update has for p, ema_update has for e: ONE expression in csrc/common.h behind the scalar kernel and the float4 loop"""
    n = 8192 + 12
    b = _buffers(n, seed=23)
    table = eng.adamw_groups([dict(begin=0, end=n, lr_scale=1.0, weight_decay=1e-2, frozen=False)], n)
    for w in WEIGHTS.values():
        for mx in (0.0, 1e9):       # no clipping at all / a coefficient of exactly 1 (the two norms are summed in different fixed orders)
            a = _run(eng, b, 2, w=w, max_grad_norm=mx)
            c = _run(eng, b, 2, w=w, max_grad_norm=mx, table=table, n_groups=1, weight_decay=0.77)
            assert all(torch.equal(a[k], c[k]) for k in "pmve"), (w, mx)
    table.close()


def test_ema_argument_errors_launch_nothing(eng):
    groups, n = _groups()
    table = eng.adamw_groups(groups, n)
    b = _buffers(n, seed=24)
    P, G, M, V, E = (_dev(b[k], 0) for k in "pgmve")
    E1 = _dev(b["e"], 1)
    hp = _lib.AdamWHParams(1e-3, 0.9, 0.95, 1e-8, 1e-2, 1.0, 1.0)

    def refused(match, ema, w, tab):
        rc = eng.lib.fv_adamw_clip_step_ema(eng.h, P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), ema, C.c_float(w), n, C.byref(hp),
                                            tab.handle() if tab is not None else None, 1, None, None, None)
        msg = eng.lib.fv_last_error(eng.h).decode()
        assert rc == -1 and match in msg, (match, rc, msg)
        torch.cuda.synchronize()
        for k, t in zip("pgmv", (P, G, M, V)):
            assert torch.equal(t.cpu(), b[k]), (match, k)
        assert torch.equal(E.cpu(), b["e"]) and torch.equal(E1.cpu(), b["e"]), match

    for tab in (None, table):
        refused("ema is null", None, 0.5, tab)
        refused("ema aliases flat_params", P.data_ptr(), 0.5, tab)
        refused("ema aliases m", M.data_ptr(), 0.5, tab)
        refused("ema aliases v", V.data_ptr(), 0.5, tab)
        for bad in (-0.25, 1.5, float("nan"), float("inf")):
            refused("ema_weight", E.data_ptr(), bad, tab)
    refused("ema must be 16-byte aligned", E1.data_ptr(), 0.5, table)
    with pytest.raises(FastVLAHipError, match="ema_weight") as ei:      # ... and through the binding
        eng.adamw_step(P, G, M, V, 1, lr=1e-3, ema=E, ema_weight=2.0)
    assert ei.value.status == -1
    with pytest.raises(ValueError, match="ema_weight"):
        eng.adamw_step(P, G, M, V, 1, lr=1e-3, ema=E)
    table.close()


# ------------------------------------------------------------------------------------------------------------------ step level: the policy's training steps
# Head-only runs on the `tiny` preset.  The decoder training kernels need head_dim 64 or 128 (fv_train_begin), which `tiny` (head_dim 32) does not have: the
# unfrozen modes run on `small`, the smallest preset that trains, as every other unfrozen policy test does.  B = 2, prompts of <= 8 tokens.
EMA_OPTS = dict(decay=0.999, warmup=True, update_after=1)
MODES = {
    "head": dict(model="tiny:77", K=1, enable=None),
    "head_chunk3": dict(model="tiny:77", K=3, enable=None),
    "full_decoder": dict(model="small:41", K=1, enable={}),
    "lora_groups_frozen": dict(model="small:41", K=1, enable=dict(lora_rank=4, lora_alpha=8.0, lora_plus_ratio=16, no_decay=("vectors",), freeze=("projector",))),
    "tower": dict(model="small:41", K=1, enable=dict(tower=True)),
}


def _policy(mode, ema=True, seed=31):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    spec = MODES[mode]
    torch.manual_seed(seed)
    cfg = FastVLAConfig(vlm_model_name=f"synthetic:{spec['model']}", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=spec["enable"] is None)
    pol = FastVLAPolicy(cfg, chunk_size=spec["K"], action_loss="l1" if spec["K"] > 1 else "mse").to(DEV)
    pol.train()
    if spec["enable"] is not None:
        pol.enable_backbone_training(**spec["enable"])
    if ema:
        pol.enable_ema(**EMA_OPTS)
    return pol


def _batch(K=1, B=2, seed=6):
    g = torch.Generator().manual_seed(seed)
    return {"images": torch.rand(B, 3, 96, 128, generator=g).to(DEV), "states": torch.randn(B, 14, generator=g).to(DEV),
            "actions": (torch.randn(B, K, 14, generator=g) if K > 1 else torch.randn(B, 14, generator=g)).to(DEV), "tasks": ["pick up the red cube", "open the drawer"][:B]}


def _state(pol):
    """(p, m, v) of the run, CPU copies"""
    live = pol._ema_live()
    return tuple(t.detach().cpu().clone() for t in (live, pol._opt_state["m"], pol._opt_state["v"]))


def _close(*pols):
    for p in pols:
        p.model.backbone.engine().close()


@pytest.mark.parametrize("mode", list(MODES))
def test_training_steps_keep_the_average_and_compute_what_they_computed(mode, monkeypatch):
    """4 optimiser updates over 6 micro-batches (two updates close a grad_accum_steps = 2 window), warmup with update_after = 1: after every update the
    average obeys the op-level bound from the device's previous average and new parameters with the scheduled weight (1 at the first update: a bitwise copy);
    a micro-batch that does not sync leaves it bit for bit; loss, p, m, v are bitwise those of the same run with EMA off"""
    for k in ("FASTVLA_EMA_DECAY", "FASTVLA_EMA_WARMUP", "FASTVLA_EMA_UPDATE_AFTER"):
        monkeypatch.delenv(k, raising=False)
    K = MODES[mode]["K"]
    a, b = _policy(mode, ema=True), _policy(mode, ema=False)
    opts = ema_mod.normalize_options(**EMA_OPTS)
    assert a.ema_enabled and not b.ema_enabled
    if MODES[mode]["enable"] is not None:       # the trainable buffer exists: so does the average, a bitwise copy
        assert torch.equal(a.ema_shadow, a._ema_live()) and a.ema_shadow.data_ptr() != a._ema_live().data_ptr()
    plan = [(1, 11), (2, 12), (2, 13), (1, 14), (2, 15), (2, 16)]       # (grad_accum_steps, batch seed)
    kw = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    updates, shadow_prev = 0, None       # (the first micro-batch closes an update: shadow_prev is set before a micro-step that does not)
    for k, seed in plan:
        batch = _batch(K, seed=seed)
        oa = a.fused_train_step(batch, grad_accum_steps=k, **kw)
        ob = b.fused_train_step(batch, grad_accum_steps=k, **kw)
        torch.cuda.synchronize()
        assert oa["synced"] == ob["synced"] and torch.equal(oa["loss"], ob["loss"]) and "ema_weight" in oa and "ema_weight" not in ob
        shadow = a.ema_shadow.detach().cpu().clone()
        if oa["synced"]:
            updates += 1
            w = ema_mod.ema_weight(opts, updates)
            assert oa["ema_weight"] == w and a._opt_state["step"] == updates
            if updates == 1:
                assert w == 1.0 and torch.equal(shadow, _state(a)[0])          # update 1 <= update_after: the average IS the live weights
            else:
                assert 0.0 < w < 1.0
                check_ema(f"{mode} update {updates}", shadow, shadow_prev, _state(a)[0], w)
        else:
            assert torch.equal(shadow, shadow_prev), f"{mode}: an accumulation micro-step touched the average"
        shadow_prev = shadow
    assert updates == 4 and a._ema["updates"] == 4
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y), f"{mode}: p, m or v differs from the run without EMA"
    assert not torch.equal(a.ema_shadow, a._ema_live())
    if mode == "lora_groups_frozen":       # the frozen projector: parameters and average still the initial bits, both
        un = a._unfrozen
        groups, _ = un.param_groups(1e-2)
        fr = [g for g in groups if g["frozen"]]
        assert fr
        for g in fr:
            assert torch.equal(a.ema_shadow[g["begin"]: g["end"]], un.trainable[g["begin"]: g["end"]])
    a.disable_ema()
    assert a.ema_shadow is None and "ema_weight" not in a.fused_train_step(_batch(K, seed=17), **kw)
    _close(a, b)


def _actions(pol, batch):
    pol.eval()
    with torch.no_grad():
        out = pol(batch["images"], batch["states"], batch["tasks"]).clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", ["head", "full_decoder", "lora_groups_frozen"])
def test_ema_weights_scope_apply_and_merge(mode):
    from test_gpu_lora import rel_l2
    K = MODES[mode]["K"]
    pol = _policy(mode)
    kw = dict(lr=2e-3, weight_decay=1e-2)
    for seed in (11, 12, 13):
        pol.fused_train_step(_batch(K, seed=seed), **kw)
    torch.cuda.synchronize()
    batch = _batch(K, seed=21)
    bb = pol.model.backbone
    if bb.splice_image_tokens:
        bb.cache_image_prefix = True      # per-image decoder prefixes are kept across calls: what the scope must not be served
    live = _actions(pol, batch)
    assert torch.equal(_actions(pol, batch), live)
    spliced = bb.splice_image_tokens
    if spliced:
        assert bb._prefix_stats["tower_runs"] == 0          # the second call was served from the image-prefix cache
    # a second policy whose trainable buffer is overwritten with the average and committed
    ref = _policy(mode, ema=False)
    if ref._ema_live() is None:
        ref.model.materialize(torch.device(DEV))
    ref._ema_live().copy_(pol.ema_shadow)
    if ref._unfrozen is not None:
        ref._unfrozen.commit()
    want = _actions(ref, batch)
    assert not torch.equal(want, live)
    live_ptr = pol._ema_live().data_ptr()
    with pol.ema_weights():
        if spliced:
            assert len(bb.__dict__.get("_prefix_cache", {})) == 0
        else:
            assert len(bb.__dict__.get("_prompt_cache", {})) == 0
        inside = _actions(pol, batch)
        if spliced:
            assert bb._prefix_stats["tower_runs"] == 2      # the prefixes cached before the scope were NOT served
        assert torch.equal(inside, want), f"{mode}: actions inside the scope differ from a policy committed from the average"
        with pol.ema_weights():                              # re-entrant: a no-op
            assert torch.equal(_actions(pol, batch), inside)
        assert pol._ema["scope"]
        sel = pol.select_action(batch["images"][0], batch["states"][0], batch["tasks"][0], torch.device(DEV))
        assert torch.equal(sel, ref.select_action(batch["images"][0], batch["states"][0], batch["tasks"][0], torch.device(DEV)))
        with pytest.raises(RuntimeError, match="ema_weights"):
            pol.fused_train_step(_batch(K, seed=14), **kw)
        if pol._unfrozen is not None and pol._unfrozen.lora is not None:
            with pytest.raises(RuntimeError, match="ema_weights"):
                pol.merge_lora()
        sd = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    assert not pol._ema["scope"] and pol._ema_live().data_ptr() == live_ptr
    after = _actions(pol, batch)
    if spliced:
        assert bb._prefix_stats["tower_runs"] == 2          # ... nor the scope's own after it
    assert torch.equal(after, live), f"{mode}: the live model changed across the scope"
    hn = pol.model._engine().head_numel()
    views = pol.model._engine().head_views(pol.ema_shadow[:hn])
    assert torch.equal(sd["model.action_head.weight"], views["action_head.weight"].cpu())          # state_dict() inside the scope held the averaged head
    pol.train()
    out = pol.fused_train_step(_batch(K, seed=14), **kw)       # training goes on after the scope
    assert out["synced"] and pol._opt_state["step"] == 4
    # apply_ema(): live <- average, bitwise, moments kept
    shadow, m0 = pol.ema_shadow.detach().clone(), pol._opt_state["m"].detach().clone()
    with pol.ema_weights():
        inside = _actions(pol, batch)
    pol.apply_ema()
    assert torch.equal(pol._ema_live(), shadow) and torch.equal(pol._opt_state["m"], m0) and torch.equal(pol.ema_shadow, shadow)
    assert torch.equal(_actions(pol, batch), inside)
    if mode == "lora_groups_frozen":
        # the export path: averaged adapters folded into the master.  tests/test_gpu_lora.py holds a merged model to 1e-5 (rel_l2 of the actions) against the
        # adapted one; the same figure here
        pol.merge_lora()
        e = rel_l2(_actions(pol, batch).cpu(), inside.cpu())
        print(f"[ema apply + merge] merged actions vs the in-scope LoRA actions: rel_l2 {e:.2e}")
        assert e <= 1e-5
    _close(pol, ref)


@pytest.mark.parametrize("mode", ["head", "full_decoder"])
def test_trainer_checkpoint_resume_and_ema_directory(mode, tmp_path, monkeypatch):
    """Trainer with EMA: 3 updates, save, resume in a fresh policy, 2 more == an uninterrupted 5-update run, bitwise in the average, the parameters and the
    moments; checkpoints/step-3-ema/ loads as a plain policy that acts like ema_weights() did at save time -- bitwise in head-only mode, within the 1e-5 of
    tests/test_gpu_train_unfrozen.py's reloaded-checkpoint comparison where the backbone travels through the file and the bf16 operand images"""
    from test_gpu_lora import rel_l2
    from vla_fastvlm.training import Trainer, TrainingConfig
    from vla_fastvlm.utils import load_policy_from_checkpoint
    for k in ("FASTVLA_EMA_DECAY", "FASTVLA_EMA_WARMUP", "FASTVLA_EMA_UPDATE_AFTER", "FASTVLA_EMA_SAVE"):
        monkeypatch.delenv(k, raising=False)
    cpu = lambda b: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()}  # noqa: E731
    data = [cpu(_batch(seed=s)) for s in (31, 32, 33, 34, 35)]
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1, eval_steps=1000, seed=1)
    a = _policy(mode)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=5, **tkw)).fit()
    b = _policy(mode)
    tb = Trainer(b, data[:3], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=3, max_steps=5, **tkw))
    tb.num_training_steps = 5
    tb.fit()
    torch.cuda.synchronize()
    ck = tmp_path / "b" / "checkpoints" / "step-3"
    opt = torch.load(ck / "optimizer.pt", map_location="cpu")
    assert sorted(opt["ema"]) == ["options", "shadow", "updates"] and opt["ema"]["options"] == ema_mod.normalize_options(**EMA_OPTS) and opt["ema"]["updates"] == 3
    assert torch.equal(opt["ema"]["shadow"], b.ema_shadow.cpu())
    # the weight files of the checkpoint are the LIVE weights
    sd = torch.load(ck / "policy_state_dict.pt", map_location="cpu")
    assert torch.equal(sd["model.action_head.weight"], b.model.action_head.weight.detach().cpu())
    log = [__import__("json").loads(ln) for ln in (tmp_path / "b" / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert [r["train/ema_weight"] for r in log] == [ema_mod.ema_weight(opt["ema"]["options"], t) for t in (1, 2, 3)]
    # <suffix>-ema/: the weight files only, a plain deployable policy of the averaged weights
    ed = tmp_path / "b" / "checkpoints" / "step-3-ema"
    assert (ed / "policy_state_dict.pt").is_file() and (ed / "policy_config.json").is_file() and not (ed / "optimizer.pt").exists()
    batch = _batch(seed=21)
    with b.ema_weights():
        want = _actions(b, batch)
    dep = load_policy_from_checkpoint(str(ed)).to(DEV)
    got = _actions(dep, batch)
    if mode == "head":
        assert torch.equal(got, want)
    else:
        e = rel_l2(got.cpu(), want.cpu())
        print(f"[ema checkpoint {mode}] step-3-ema reloaded vs ema_weights() at save time: actions rel_l2 {e:.2e}")
        assert e <= 1e-5
    assert not torch.equal(want, _actions(b, batch))
    # resume: a fresh policy with the same EMA options continues the average bit for bit
    c = _policy(mode, seed=99 if mode == "head" else 31)
    tc = Trainer(c, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=5, resume_from=str(ck), **tkw))
    tc.num_training_steps = 5
    tc.fit()
    torch.cuda.synchronize()
    assert tc.update_step == 5 and c._opt_state["step"] == 5 and c._ema["updates"] == 5
    assert torch.equal(c.ema_shadow, a.ema_shadow), "the resumed average differs from the uninterrupted run's"
    for x, y in zip(_state(c), _state(a)):
        assert torch.equal(x, y)
    # other EMA options do not resume; a run without EMA warns and drops the record; a run with EMA resumes a record without one from the live weights
    d = _policy(mode, ema=False)
    d.enable_ema(decay=0.99, warmup=False, update_after=0)
    td = Trainer(d, data[3:], None, TrainingConfig(output_dir=str(tmp_path / "d"), save_steps=1000, max_steps=5, resume_from=str(ck), **tkw))
    with pytest.raises(ValueError) as ei:
        td.fit()
    assert "'decay': 0.999" in str(ei.value) and "'decay': 0.99," in str(ei.value)
    e_ = _policy(mode, ema=False)
    te = Trainer(e_, data[3:4], None, TrainingConfig(output_dir=str(tmp_path / "e"), save_steps=1, max_steps=4, resume_from=str(ck), **tkw))
    te.num_training_steps = 5
    with pytest.warns(UserWarning, match="EMA off"):
        te.fit()
    assert not e_.ema_enabled
    plain = torch.load(tmp_path / "e" / "checkpoints" / "step-4" / "optimizer.pt", map_location="cpu")
    assert "ema" not in plain and not (tmp_path / "e" / "checkpoints" / "step-4-ema").exists()
    f = _policy(mode)
    tf = Trainer(f, [], None, TrainingConfig(output_dir=str(tmp_path / "f"), save_steps=1000, max_steps=5, resume_from=str(tmp_path / "e" / "checkpoints" / "step-4"), **tkw))
    tf.num_training_steps = 5
    tf.fit()
    assert torch.equal(f.ema_shadow, f._ema_live()) and torch.equal(f._ema_live(), e_._ema_live()) and f._ema["updates"] == 0
    _close(a, b, c, d, e_, f, dep)


def test_trainer_evaluates_the_averaged_weights(tmp_path, monkeypatch):
    from vla_fastvlm.training import Trainer, TrainingConfig
    for k in ("FASTVLA_EMA_DECAY", "FASTVLA_EMA_WARMUP", "FASTVLA_EMA_UPDATE_AFTER", "FASTVLA_EMA_SAVE"):
        monkeypatch.delenv(k, raising=False)
    cpu = lambda b: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()}  # noqa: E731
    data, ev = [cpu(_batch(seed=s)) for s in (31, 32, 33)], [cpu(_batch(seed=41))]
    monkeypatch.setenv("FASTVLA_EMA_DECAY", "0.9")           # the twin alone switches it on for Trainer
    pol = _policy("head", ema=False)
    tr = Trainer(pol, data, ev, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=1000, max_steps=3, num_epochs=1, learning_rate=3e-3, warmup_ratio=0.0,
                                               logging_steps=1000, eval_steps=1000, seed=1))
    assert pol.ema_enabled and pol._ema["options"] == {"decay": 0.9, "warmup": True, "update_after": 0}
    tr.evaluate_live = True
    tr.fit()
    m = tr.evaluate()
    pol.eval()
    with torch.no_grad():
        live = float(pol.compute_loss({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ev[0].items()})["mse"])
        with pol.ema_weights():
            avg = float(pol.compute_loss({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ev[0].items()})["mse"])
    assert m["eval/mse"] == avg and m["eval/mse_live"] == live and avg != live
    tr.evaluate_live = False
    assert sorted(tr.evaluate()) == ["eval/mse"]
    _close(pol)


def test_off_by_default_digests_equal_the_parent_builds(monkeypatch):
    """With FASTVLA_EMA_* unset, sha256 of (p, m, v) after 3 head-only and 3 LoRA updates equals what the PARENT commit's build gave on the same GPU model
    (tools/ema_bench.py --digest run on a checkout of the parent; recorded in profiles/ema_bench.json)."""
    import importlib.util
    import json
    from pathlib import Path
    for k in ("FASTVLA_EMA_DECAY", "FASTVLA_EMA_WARMUP", "FASTVLA_EMA_UPDATE_AFTER"):
        monkeypatch.delenv(k, raising=False)
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("ema_bench", root / "tools" / "ema_bench.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rec = json.loads((root / "profiles" / "ema_bench.json").read_text())["digests"]
    got = tool.default_path_digests()
    print("[ema off-by-default digests]", got)
    assert set(rec["parent"]) == set(got) == {"head_only", "lora_rank4"}
    assert got == rec["parent"], "a run that does not switch EMA on no longer computes the parent's bits"
