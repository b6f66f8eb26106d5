"""-m gpu: the engine's FULL-SIZE dispatch chain against the CPU oracle (BASELINE.json configs C1, C2, C4 shapes).

The reduced presets of test_gpu_e2e.py take other kernels than the real model does (convffn_kernel<32/64/128> instead of
<96,4>/<192,4>/<384,2>, gemm_kernel<128> instead of gemm256_kernel + split-K, no pwconv_kernel, no dwconv_s2_mfma at
256^2, no stem_fused at 1024^2, no attention32_kernel at 1024 tokens x 24 heads), so these tests run `fastvlm-0.5b` and the
`fastvlm-7b` decoder at their real dimensions, on the same seeded weights and inputs as the oracle:

  * tower + projector, B=2, 336^2 -> 1024^2, with per-stage taps so a failure names the stage
    (reference call site: src/vla_fastvlm/model/fastvlm_adapter.py:533; oracle: oracle/fastvit_hd.py, parity-unpinned);
  * C1 (B=4, 32-token prompt): actions, loss, the 12 head gradients and one clip+AdamW step, literal and spliced
    (reference: fastvlm_adapter.py:501-560, fastvla/fastvlm_with_expert.py:40-54, training/trainer.py:171-182);
  * the 7B decoder at full width on 4 layers vs the oracle, and the WHOLE 7B preset at B=16 through size-independent
    properties (finite, deterministic, batch rows independent of their neighbours);
  * round 3: every one of the tower's 51 units (stem, 44 blocks, 2 RepCPEs, 4 PatchEmbeds) TEACHER-FORCED -- the fp32 oracle
    unit is fed the engine's own input of that unit, so nothing is amplified and the bound is the op-level 4e-3; C2's batch
    (B=64: rows 0-3 against the B=4 run, replays bit-identical, 32-bit offsets at their largest); C3's per-rank shape (B=32
    train step with dropout 0.1, the kernel's mask recovered and handed to the oracle); C5's per-rank shape (7B, B=8, a
    two-camera LeRobot batch: first-camera semantics of lerobot_fastvla/modeling_fastvla.py:82).

Tolerances (north_star: actions/loss within 1e-3 relative of the fp32 reference):
  * tower maps / embeddings / image tokens: the product keeps tower activations in bf16 (as the reference's own default
    mixed_precision="bf16" does).  The oracle has a bf16-faithful mode (same graph, a round-to-bf16 wherever the product's
    kernels round: oracle/fastvit_hd.py); its deviation from the fp32 mode is measured per tap in the test (3e-3 after the stem,
    2.5e-2 after 38 blocks: rounding noise amplified by the random-weight network) and the engine must stay within 1.25x of it
    against the fp32 oracle and 1.1x against the bf16-faithful one (independent realisations of the same rounding noise would
    sit at 1.41x), plus absolute caps on the first taps (stem 3e-3, stage0 5e-3) where nothing has been amplified yet;
  * literal C1: actions, loss <= 1e-3; gradients <= 1e-3 of each tensor's max; parameters after the step to 2e-6 absolute
    (lr 1e-4, so a sign flip of a ~0 gradient entry moves a parameter by at most 2e-4 * ... -- see the test);
  * spliced C1: the image tokens carry the tower's bf16 rounding into the decoder.  Same self-calibrated bound: the oracle with
    the bf16-faithful tower moves its OWN actions by d (1.7e-2 here) against the all-fp32 oracle; the engine must be within
    1.25 d of the fp32 oracle and 1.1 d of the bf16-faithful one (stated, not the 1e-3 bar: the reference itself never runs
    this mode -- SURVEY.md fact 5 -- and under its default bf16 autocast its own tower output moves by as much).
"""
import numpy as np
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, check_close, rel_l2, worst_row  # noqa: E402
from fastvla_hip import FastVLAEngine, arch, weights  # noqa: E402
from oracle import fastvit_hd, head, policy, preprocess, qwen2  # noqa: E402


# bf16 activations through 44 blocks against the fp32 graph: 3e-3 after the stem .. 2.7e-2 after the last stage -- and the
# ORACLE's own bf16-faithful mode deviates from its fp32 mode by exactly those amounts (measured in the test, printed).  The
# tests therefore bound the engine by the policy deviation measured on the spot: a kernel or wiring bug adds error on top of
# the policy's, a correct engine does not.
TOWER_TOL_FP32 = 4e-2


def _cfgs(m):
    tc = fastvit_hd.TowerCfg(layers=m.tower.layers, dims=m.tower.dims, mlp_ratio=m.tower.mlp_ratio,
                             head_dim=m.tower.head_dim, attn_stages=m.tower.attn_stages)
    lc = qwen2.Qwen2Cfg(hidden=m.llm.hidden, layers=m.llm.layers, heads=m.llm.heads, kv_heads=m.llm.kv_heads,
                        head_dim=m.llm.head_dim, inter=m.llm.inter, vocab=m.llm.vocab, rope_theta=m.llm.rope_theta,
                        rms_eps=m.llm.rms_eps)
    return tc, lc


@pytest.fixture(scope="module")
def full():
    """fastvlm-0.5b at its real dimensions (tower at 1024^2, 24-layer decoder, 151936-row embedding), default head dims."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m = arch.preset("fastvlm-0.5b")
    w = weights.init_backbone(m, seed=2024)
    eng = FastVLAEngine(m, state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024, max_batch=64, max_text_tokens=64, llm_precision=1)
    eng.load_weights(w)
    yield m, w, eng
    eng.close()


# per-sample bound on the actions / pooled feature by decoder policy: 1 (the default) holds north_star's 1e-3 on EVERY row with margin;
# 2 (opt-in) holds it on the batch's rel-L2 but its worst row was measured at 1.1e-3 (C1) -- which is why it is not the default
WORST_ROW_TOL = {1: 1e-3, 2: 2e-3, 5: 1e-3}


@pytest.fixture(scope="module", params=[1, 2, 5], ids=["policy1", "policy2-optin", "policy5-hi-lo8"])
def fullp(request, full):
    """The same model and weights under BOTH decoder policies the product ships for the 0.5B decoder: 1 (split-bf16 everywhere:
    arch.default_llm_precision, what bench.py and every FastVLMBackbone run) and the opt-in 2 (fp16 gate/up/down).
    VERDICT r3 #1: C1 / C2 / C3 are asserted in the mode the headline number is measured in, row by row."""
    m, w, eng1 = full
    if request.param == 1:
        yield m, w, eng1
        return
    eng = FastVLAEngine(m, state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024, max_batch=64, max_text_tokens=64,
                        llm_precision=request.param)
    eng.load_weights(w)
    yield m, w, eng
    assert eng.fp16_saturations() == 0   # nothing in these runs came near the fp16 range
    eng.close()


def _head_params(lc, seed):
    shapes = head.head_shapes(lc.hidden, 14, 14, 1024, 1024)
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(*s, generator=g) / (s[-1] ** 0.5 if len(s) > 1 else 10.0))
            + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0) for k, s in shapes.items()}


def _flat_head(eng, p):
    flat = torch.zeros(eng.head_numel(), dtype=torch.float32, device=DEV)
    for k, v in eng.head_views(flat).items():
        v.copy_(p[k])
    return flat


def test_full_size_tower_per_stage(full):
    m, w, eng = full
    tc, _ = _cfgs(m)
    torch.manual_seed(11)
    img = torch.rand(2, 3, 336, 336)
    pix = eng.preprocess(img.to(DEV))
    tok, tout, taps = eng.vision_forward_taps(pix)
    torch.cuda.synchronize()
    x = pix.float().cpu()[..., :3].permute(0, 3, 1, 2).contiguous()  # the oracle sees the bf16 pixels the tower saw
    check_close(x, preprocess.letterbox(img, m.tower.image_size), rel=3e-3, amax=5e-3, what="letterbox 336->1024")
    names = ["stem"] + [f"stage{i}" for i in range(len(m.tower.dims))]
    got = {n: t.float().cpu() for n, t in zip(names, taps)}
    got["embeddings"], got["tokens"] = tout.float().cpu(), tok.cpu()
    refs = {}
    for mode in ("fp32", "bf16"):
        ref = {}
        with torch.no_grad():
            emb = fastvit_hd.tower_forward(w, x, tc, taps=ref, emulate_bf16=mode == "bf16")
            ref_tok = fastvit_hd.projector_forward(w, emb, emulate_bf16=mode == "bf16")
        ref = {n: ref[n].permute(0, 2, 3, 1) for n in names}  # NCHW -> NHWC
        ref["embeddings"], ref["tokens"] = emb, ref_tok
        refs[mode] = ref
    # what the bf16 precision policy alone does to THIS graph with THESE weights: the oracle against itself
    policy_dev = {n: rel_l2(refs["bf16"][n], refs["fp32"][n]) for n in got}
    e32 = {n: rel_l2(got[n], refs["fp32"][n]) for n in got}
    e16 = {n: rel_l2(got[n], refs["bf16"][n]) for n in got}
    print("[fastvlm-0.5b 1024^2] rel_l2 per tap  (engine vs fp32 oracle | engine vs bf16-faithful oracle | oracle bf16 vs oracle fp32)")
    for n in got:
        print(f"    {n:<11} {e32[n]:.2e} | {e16[n]:.2e} | {policy_dev[n]:.2e}")
    for n in got:  # in graph order: the first failing name is the stage that broke
        assert torch.isfinite(got[n]).all(), n
        assert policy_dev[n] <= TOWER_TOL_FP32, (n, policy_dev[n])
        assert e32[n] <= 1.25 * policy_dev[n] + 5e-4, f"tower {n}: {e32[n]:.3e} vs the fp32 oracle, the policy alone gives {policy_dev[n]:.3e}"
        assert e16[n] <= 1.10 * policy_dev[n] + 5e-4, f"tower {n}: {e16[n]:.3e} vs the bf16-faithful oracle, the policy alone gives {policy_dev[n]:.3e}"
    assert e16["stem"] <= 3e-3 and e16["stage0"] <= 5e-3  # before the noise has had 12+ blocks to amplify, the kernels are tight


def test_full_size_tower_microbatch_and_batch_rows(full):
    """size-independent property at the bench batch shape: an image's tokens do not depend on its neighbours or on the tower micro-batch
    (B = 8 in one pass == the same images four at a time).  The launchers pick tile shapes by a launch's row count; down to B = 4 every kernel
    accumulates in the same order, so the rows agree to the last bf16 rounding at most.  Below that (the control loop: one or two observations) the fused
    ConvFFN cuts its hidden units into ranges -- another fp32 summation order, <= 1 bf16 step per output (test_fused_convffn32_hidden_ranges) -- and the
    tower carries a rounding-level difference to its output as it carries its own bf16 roundings (two bf16 executions of the oracle sit 1.2e-2 apart,
    DESIGN.md section 6): one image at a time is held to that distance, not to bit equality."""
    m, w, eng = full
    torch.manual_seed(12)
    pix = eng.preprocess(torch.rand(8, 3, 336, 336).to(DEV))
    a = eng.vision_forward(pix)
    b = torch.cat([eng.vision_forward(pix[i:i + 4].contiguous()) for i in (0, 4)], dim=0)
    c = torch.cat([eng.vision_forward(pix[i:i + 1].contiguous()) for i in range(4)], dim=0)
    torch.cuda.synchronize()
    r = rel_l2(a.cpu(), b.cpu())
    r1 = rel_l2(a[:4].cpu(), c.cpu())
    print(f"[fastvlm-0.5b] B=8 in one pass vs four images at a time: identical={bool(torch.equal(a, b))} rel_l2={r:.2e}; vs one image at a time (hidden-range "
          f"ConvFFN, row-segmented depthwise pair): rel_l2={r1:.2e}")
    assert r <= 2e-3
    assert r1 <= 3e-2
    # fv_set_batch_invariant: the tower keeps the large-batch forms at every batch size -- one image at a time then agrees to the last rounding too
    eng.set_batch_invariant(True)
    try:
        d = torch.cat([eng.vision_forward(pix[i:i + 1].contiguous()) for i in range(4)], dim=0)
        torch.cuda.synchronize()
    finally:
        eng.set_batch_invariant(False)
    r2 = rel_l2(a[:4].cpu(), d.cpu())
    print(f"[fastvlm-0.5b] batch-invariant tower, one image at a time: rel_l2={r2:.2e}")
    assert r2 <= 2e-3


@pytest.mark.parametrize("splice", [False, True], ids=["literal", "splice"])
def test_c1_train_step(fullp, splice):
    """BASELINE.json configs[0] (C1): FastVLM-0.5B, bs=4, 336^2 + 32-token prompt, one training step -- under both decoder policies."""
    m, w, eng = fullp
    tc, lc = _cfgs(m)
    torch.manual_seed(21)
    B, T = 4, 32
    img = torch.rand(B, 3, 336, 336)
    ids = torch.randint(0, 151643, (B, T))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[2, 19:] = 0  # one ragged prompt
    states, tgt = torch.randn(B, 14), torch.randn(B, 14)
    p = _head_params(lc, 22)
    flat = _flat_head(eng, p)
    pooled = eng.backbone(img.to(DEV), ids, mask.sum(1), splice=splice)
    act, saved = eng.head_forward(flat, pooled, states.to(DEV))
    loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved)
    mm, vv = torch.zeros_like(flat), torch.zeros_like(flat)
    norm = torch.zeros(1, device=DEV)
    fp = flat.clone()
    eng.adamw_step(fp, grads, mm, vv, 1, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, grad_norm_out=norm)
    torch.cuda.synchronize()
    z = {k: torch.zeros_like(v) for k, v in p.items()}
    okw = dict(lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, image_size=m.tower.image_size, llm_cfg=lc, tower_cfg=tc, splice=splice,
               run_tower=splice)  # literal mode: the tower's output is dropped
    tol = 1e-3
    with torch.no_grad():
        ref = policy.train_step(w, p, z, z, 1, img, states, tgt, ids, mask, emulate_bf16_tower=splice, **okw)
        if splice:
            ref32 = policy.train_step(w, p, z, z, 1, img, states, tgt, ids, mask, **okw)
            d = rel_l2(ref["pred"], ref32["pred"])           # the policy's own effect on the actions
            r32 = rel_l2(act.cpu(), ref32["pred"])
            print(f"[C1 splice] actions: engine vs ALL-fp32 oracle {r32:.2e}; bf16-tower oracle vs fp32 oracle (policy) {d:.2e}")
            assert d <= 4e-2 and r32 <= 1.25 * d + 1e-3
            tol = 1.1 * d + 1e-3
    ra = rel_l2(act.cpu(), ref["pred"])
    rl = abs(float(loss) - float(ref["loss"])) / float(ref["loss"])
    rn = abs(float(norm) - float(ref["grad_norm"])) / float(ref["grad_norm"])
    wa = worst_row(act.cpu(), ref["pred"])
    print(f"[C1 {'splice' if splice else 'literal'} llm_precision={eng.llm_precision}] actions rel_l2={ra:.2e} worst row={wa:.2e} loss rel={rl:.2e} "
          f"grad_norm rel={rn:.2e} (tol {tol:.1e})")
    assert ra <= tol and wa <= (WORST_ROW_TOL[eng.llm_precision] if not splice else 1.5 * tol) and rl <= 2 * tol and rn <= 2 * tol
    gv = eng.head_views(grads)
    # ref["grads"] are the CLIPPED gradients; un-clip them with the oracle's own norm to compare raw gradients
    coef = min(1.0, 1.0 / (float(ref["grad_norm"]) + 1e-6))
    for k in head.HEAD_KEYS:
        rg = ref["grads"][k] / coef
        err = float((gv[k].cpu() - rg).abs().max()) / max(1e-6, float(rg.abs().max()))
        assert err <= 4 * tol, (k, err)
    # one optimiser step: |delta p| <= lr per element whatever the gradient, so compare the UPDATE, not the parameter
    for k, v in eng.head_views(fp).items():
        du = (v.cpu() - p[k])
        dr = (ref["params"][k] - p[k])
        bad = float(((du - dr).abs() > 0.05 * 1e-4 + 4 * tol * dr.abs()).float().mean())
        # Adam's first step is lr * sign-like (g / (|g| + eps)): entries whose gradient is ~0 relative to eps may differ;
        # they are a vanishing fraction
        # the fraction of entries whose gradient is small enough to flip grows with the gradient noise (splice: tol ~ 2e-2)
        assert bad <= max(2e-3, 1.5 / du.numel(), 0.5 * tol), (k, bad)


@pytest.mark.parametrize("prec,tol", [(1, 3e-4), (2, 1e-3)], ids=["split-bf16", "fp16-mlp"])
def test_7b_decoder_full_width_four_layers(prec, tol):
    """FastVLM-7B decoder geometry at FULL width (3584 hidden, 28 q / 4 kv heads of 128, inter 18944), 4 layers, weights
    streamed tensor by tensor onto the device (fv_load_weights_cb), vs the fp32 oracle on the same tensors -- in both parity
    modes of the decoder (llm_precision 1: split-bf16 everywhere; 2: the per-GEMM budget, fp16 gate/up/down)."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    llm = arch.LLMConfig(hidden=3584, layers=4, heads=28, kv_heads=4, head_dim=128, inter=18944, vocab=8192)
    m = arch.ModelConfig("7b-4layer", llm, arch.preset("tiny").tower)
    prov = weights.stream_backbone(m, seed=5, device=DEV)
    asked = []

    def provider(name):
        asked.append(name)
        return prov(name)

    eng = FastVLAEngine(m, hidden_dim=64, fusion_dim=64, max_batch=4, max_text_tokens=32, llm_precision=prec)
    eng.load_weights_streaming(provider)
    lc = qwen2.Qwen2Cfg(hidden=3584, layers=4, heads=28, kv_heads=4, head_dim=128, inter=18944, vocab=8192)
    w = {n: prov(n).float().cpu() for n in asked if n.startswith("model.") and not n.startswith("model.vision_tower") and not n.startswith("model.mm_projector")}
    torch.manual_seed(4)
    B, T = 2, 24
    ids = torch.randint(0, 8192, (B, T))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, 15:] = 0
    with torch.no_grad():
        ref = qwen2.llm_pooled(w, ids, mask, lc)
    got = eng.llm_pooled(ids, mask.sum(1))
    torch.cuda.synchronize()
    r, _ = check_close(got.cpu(), ref, rel=tol, amax=10 * tol, what=f"7B-width 4-layer pooled (llm_precision={prec})")
    print(f"[7b-4layer llm_precision={prec}] pooled rel_l2={r:.2e}")
    eng.close()


def test_1p5b_decoder_full_width_four_layers():
    """FastVLM-1.5B decoder geometry at full width (Qwen2-1.5B: 1536 hidden, 12 q / 2 kv heads of 128, inter 8960), 4 of its 28
    layers, vs the fp32 oracle -- the reference's third model size (`--model-id apple/FastVLM-1.5B`); GQA ratio 6 and a
    hidden size that is not a multiple of 256 take other tile paths than 0.5B and 7B."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    full = arch.preset("fastvlm-1.5b").llm
    llm = arch.LLMConfig(hidden=full.hidden, layers=4, heads=full.heads, kv_heads=full.kv_heads, head_dim=full.head_dim, inter=full.inter, vocab=8192)
    m = arch.ModelConfig("1.5b-4layer", llm, arch.preset("tiny").tower)
    prov = weights.stream_backbone(m, seed=6, device=DEV)
    asked = []

    def provider(name):
        asked.append(name)
        return prov(name)

    eng = FastVLAEngine(m, hidden_dim=64, fusion_dim=64, max_batch=4, max_text_tokens=64, llm_precision=1)
    eng.load_weights_streaming(provider)
    lc = qwen2.Qwen2Cfg(hidden=llm.hidden, layers=4, heads=llm.heads, kv_heads=llm.kv_heads, head_dim=llm.head_dim, inter=llm.inter, vocab=8192)
    w = {n: prov(n).float().cpu() for n in asked if n.startswith("model.") and not n.startswith("model.vision_tower") and not n.startswith("model.mm_projector")}
    torch.manual_seed(7)
    B, T = 4, 64
    ids = torch.randint(0, 8192, (B, T))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, 40:] = 0
    mask[3, 1:] = 0
    with torch.no_grad():
        ref = qwen2.llm_pooled(w, ids, mask, lc)
    got = eng.llm_pooled(ids, mask.sum(1))
    torch.cuda.synchronize()
    r, _ = check_close(got.cpu(), ref, rel=3e-4, amax=3e-3, what="1.5B-width 4-layer pooled (split-bf16)")
    print(f"[1.5b-4layer] pooled rel_l2={r:.2e}")
    eng.close()


@pytest.fixture(scope="module")
def lr7b():
    """The whole fastvlm-7b preset behind the LeRobot plugin surface (policy.type=fastvla): a two-camera aloha-shaped feature
    map, weights streamed onto the device tensor by tensor (fv_load_weights_cb) -- the engine C4 and C5 run on."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import FeatureType, PolicyFeature
    feats = {"observation.images.top": PolicyFeature(FeatureType.VISUAL, (3, 336, 336)),
             "observation.images.wrist": PolicyFeature(FeatureType.VISUAL, (3, 336, 336)),
             "observation.state": PolicyFeature(FeatureType.STATE, (14,))}
    cfg = LRConfig(vlm_model_name="synthetic:fastvlm-7b:7", input_features=feats,
                   output_features={"action": PolicyFeature(FeatureType.ACTION, (14,))})
    torch.manual_seed(9)
    pol = LRPolicy(cfg).to(DEV)
    pol.model.materialize(torch.device(DEV))
    yield pol
    pol.model.backbone.engine().close()


def test_7b_whole_preset_properties(lr7b):
    """BASELINE.json configs[3] (C4) shape: the whole fastvlm-7b preset (28 layers, 152064-row embedding, 1024^2 tower),
    B=16, 64-token prompts.  No CPU oracle finishes this in test time, so the checks are the size-independent ones:
    finite outputs of the right shape, bit-identical replays, and rows that do not depend on their batch neighbours."""
    eng = lr7b.model.backbone.engine()
    m = eng.model
    torch.manual_seed(8)
    B, T = 16, 64
    img = torch.rand(B, 3, 336, 336, device=DEV)
    ids = torch.randint(0, 151643, (B, T))
    lens = torch.full((B,), T)
    lens[3] = 40
    lc = _cfgs(m)[1]
    flat = _flat_head(eng, _head_params(lc, 9))
    states = torch.randn(B, 14, device=DEV)
    outs = []
    for _ in range(2):
        pooled = eng.backbone(img, ids, lens, splice=False)
        act, _ = eng.head_forward(flat, pooled, states)
        torch.cuda.synchronize()
        outs.append((pooled.clone(), act.clone()))
    pooled, act = outs[0]
    assert pooled.shape == (B, 3584) and act.shape == (B, 14)
    assert torch.isfinite(pooled).all() and torch.isfinite(act).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(pooled.std()) > 1e-3  # not a collapsed / zeroed feature
    # rows 3 (ragged) and 5 alone: the GEMM tiling differs with M (other kernels, split-K on or off), the numbers must not
    sub = torch.tensor([3, 5])
    p2 = eng.llm_pooled(ids[sub], lens[sub])
    torch.cuda.synchronize()
    r = rel_l2(p2.cpu(), pooled[sub].cpu())
    print(f"[fastvlm-7b B=16, llm_precision={eng.llm_precision}] pooled std={float(pooled.std()):.3f} rows-alone rel_l2={r:.2e}")
    # another tile shape accumulates K in another order: the last bits of an fp32 sum then round differently into the next GEMM's
    # operand -- 16 significant bits in mode 1, 11 (fp16) on the MLP in mode 2 (the policy default), through 28 layers
    assert r <= (2e-4 if eng.llm_precision == 1 else 1e-3)
    # spliced prefill at 7B width on 2 images: 256 + 64 tokens per row, finite and deterministic
    tok = eng.vision_forward(eng.preprocess(img[:2]))
    ps = eng.llm_pooled(ids[:2], lens[:2], tok)
    ps2 = eng.llm_pooled(ids[:2], lens[:2], tok)
    torch.cuda.synchronize()
    assert torch.isfinite(tok).all() and torch.isfinite(ps).all() and torch.equal(ps, ps2)


class _StreamedLLM:
    """The oracle's weight dict for a decoder too large to hold in fp32 (7B: 30 GB): every tensor is REGENERATED by name when
    oracle.qwen2 asks for it (fastvla_hip.weights.llm_tensor: seeded by run seed + tensor name, the same draw the engine's streaming
    loader packed) and dropped after use, so the largest live object is one 18944 x 3584 fp32 matrix."""

    def __init__(self, llm, seed, device):
        self.llm, self.seed, self.device, self.asked = llm, seed, device, 0

    def __getitem__(self, name):
        t = weights.llm_tensor(self.llm, name, self.seed, self.device)
        if t is None:
            raise KeyError(name)
        self.asked += 1
        return t.cpu().float()


def test_7b_full_depth_against_layer_streamed_oracle(lr7b):
    """VERDICT r3 missing #2 / next #1-iii: the WHOLE FastVLM-7B decoder (28 layers, hidden 3584, 28 q / 4 kv heads of 128, inter 18944,
    152064-row embedding) against the fp32 oracle -- not 4 of its layers.  The oracle streams its weights layer by layer (_StreamedLLM);
    B = 2, T = 24 (one ragged row) is ~0.6 TFLOP of CPU work.  Call site: src/vla_fastvlm/model/fastvlm_adapter.py:533 (28 decoder layers
    + final norm), pooling :551-559.  The preset's default policy (1, split-bf16 everywhere) is held to 3e-4 on the pooled feature and
    1e-3 on the actions, worst row included; policy 2's number on the SAME inputs is measured on a second engine and printed (it is the
    evidence arch.default_llm_precision keeps 7B on policy 1: DESIGN.md section 6)."""
    eng = lr7b.model.backbone.engine()
    m = eng.model
    assert eng.llm_precision == 1 and m.llm.layers == 28 and m.llm.hidden == 3584
    seed = lr7b.model.backbone._weights_source[1]
    lc = _cfgs(m)[1]
    torch.manual_seed(17)
    B, T = 2, 24
    ids = torch.randint(0, 151643, (B, T))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, 15:] = 0
    states = torch.randn(B, 14)
    p = _head_params(lc, 18)
    sw = _StreamedLLM(m.llm, seed, DEV)
    with torch.no_grad():
        ref_pooled = qwen2.llm_pooled(sw, ids, mask, lc)
        ref_act = head.head_forward(p, ref_pooled, states)
    assert sw.asked == 2 + 12 * 28 and torch.isfinite(ref_pooled).all()
    out = {}
    for prec in (1, 2, 5):
        e = eng
        if prec != 1:
            e = FastVLAEngine(m, state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024, max_batch=4, max_text_tokens=64, llm_precision=prec)
            e.load_weights_streaming(weights.stream_backbone(m, seed=seed, device=DEV))
        pooled = e.llm_pooled(ids, mask.sum(1))
        act, _ = e.head_forward(_flat_head(e, p), pooled, states.to(DEV))
        torch.cuda.synchronize()
        out[prec] = (rel_l2(pooled.cpu(), ref_pooled), worst_row(pooled.cpu(), ref_pooled), rel_l2(act.cpu(), ref_act), worst_row(act.cpu(), ref_act))
        if prec != 1:
            assert e.fp16_saturations() == 0
            e.close()
    print("[fastvlm-7b FULL DEPTH (28 layers) B=2 T=24 vs layer-streamed fp32 oracle] (pooled rel_l2, pooled worst row, actions rel_l2, actions worst row):  " +
          "  ".join(f"llm_precision={k}: " + ", ".join(f"{x:.2e}" for x in v) for k, v in out.items()))
    assert out[1][0] <= 3e-4 and out[1][1] <= 3e-4 and out[1][2] <= 1e-3 and out[1][3] <= 1e-3
    assert all(x == x for x in out[2])   # policy 2: recorded, finite
    assert out[5][0] <= 1e-3 and out[5][2] <= 1e-3   # policy 5 (bf16 hi + fp8 lo): inside the bar on the batch norm; its worst rows are printed


def test_c5_rank_shape_two_camera_train_step_7b(lr7b):
    """BASELINE.json configs[4] (C5) per-rank shape through the LeRobot surface: fastvlm-7b, B=8, TWO 336^2 cameras (stacked
    over two timesteps), 64-token task strings.  `forward(batch)` -> (loss, {"loss","mse"}) with Dropout(0.1) + backward reaches
    all 12 head tensors; reference semantics lerobot_fastvla/modeling_fastvla.py:81-107: only the FIRST visual key and the LAST
    timestep feed the backbone.  In literal mode no pixel reaches the actions at all, so the camera check runs
    with the image tokens spliced in: actions are bit-identical when the second camera (or the older frame) changes, and
    change when the first camera's last frame does."""
    pol = lr7b
    g = torch.Generator().manual_seed(61)
    B = 8
    batch = {"observation.images.top": torch.rand(B, 2, 3, 336, 336, generator=g).to(DEV),
             "observation.images.wrist": torch.rand(B, 2, 3, 336, 336, generator=g).to(DEV),
             "observation.state": torch.randn(B, 2, 14, generator=g).to(DEV),
             "action": torch.randn(B, 1, 14, generator=g).to(DEV),
             "task": [f"insert the peg into socket number {i} with the left arm, then hold it still" for i in range(B)]}
    pol.train()
    pol.zero_grad()
    loss, info = pol.forward(batch)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and info["loss"] == info["mse"] == pytest.approx(float(loss))
    for prm in pol.model.head_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all()
    assert float(pol.model.fusion[0].weight.grad.abs().max()) > 0
    assert pol.model.fusion[0].weight.shape == (1024, 3584 + 1024)   # 7B: fusion.0 is (3584 + 1024) -> 1024
    bb = pol.model.backbone
    bb.splice_image_tokens = True
    try:
        pol.reset()
        a0 = pol.select_action(batch).clone()
        pol.reset()
        a0b = pol.select_action(batch).clone()
        other = dict(batch)
        other["observation.images.wrist"] = torch.rand(B, 2, 3, 336, 336, generator=g).to(DEV)
        top = batch["observation.images.top"].clone()
        top[:, 0] = torch.rand(B, 3, 336, 336, generator=g).to(DEV)      # the OLDER frame of camera 1
        other["observation.images.top"] = top
        pol.reset()
        a1 = pol.select_action(other).clone()
        top2 = batch["observation.images.top"].clone()
        top2[:, -1] = torch.rand(B, 3, 336, 336, generator=g).to(DEV)    # the frame the policy does look at
        pol.reset()
        a2 = pol.select_action({**batch, "observation.images.top": top2}).clone()
        torch.cuda.synchronize()
    finally:
        bb.splice_image_tokens = False
    assert a0.shape == (B, 14) and torch.isfinite(a0).all()
    assert torch.equal(a0, a0b) and torch.equal(a0, a1) and not torch.equal(a0, a2)
    print(f"[C5 rank shape: 7B, B=8, 2 cams] loss={float(loss):.4f}; actions move by {rel_l2(a2.cpu(), a0.cpu()):.2e} when camera 1's last frame changes")


def test_spliced_select_action_does_not_depend_on_the_batch_with_defaults():
    """VERDICT r5 #6 (reference call site: lerobot_fastvla/modeling_fastvla.py:119-125, one observation per env step): in splice mode the action of ONE observation
    through `select_action` equals its row of a B = 8 call to <= 2e-3 with DEFAULT settings -- the host side tells the engine that the tower tokens are consumed and
    the tower then keeps one set of kernel forms at every batch size (without that the B <= 2 hidden-range / K-range forms sit 1.7e-2 away at the tower's output).
    In literal mode the tokens are dropped, the fast small-batch forms stay, and the actions cannot depend on the pixels at all."""
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import FeatureType, PolicyFeature
    assert os.environ.get("FASTVLA_BATCH_INVARIANT") in (None, ""), "this test is about the defaults"
    feats = {"observation.images.top": PolicyFeature(FeatureType.VISUAL, (3, 336, 336)), "observation.state": PolicyFeature(FeatureType.STATE, (14,))}
    cfg = LRConfig(vlm_model_name="synthetic:fastvlm-0.5b:13", input_features=feats, output_features={"action": PolicyFeature(FeatureType.ACTION, (14,))})
    torch.manual_seed(14)
    pol = LRPolicy(cfg).to(DEV)
    pol.model.materialize(torch.device(DEV))
    bb, eng = pol.model.backbone, pol.model.backbone.engine()
    g = torch.Generator().manual_seed(62)
    B = 8
    batch = {"observation.images.top": torch.rand(B, 3, 336, 336, generator=g).to(DEV), "observation.state": torch.randn(B, 14, generator=g).to(DEV),
             "task": [f"put object {i} into the bin" for i in range(B)]}

    def one_at_a_time(n):
        rows = []
        for i in range(n):
            pol.reset()
            rows.append(pol.select_action({k: v[i:i + 1] for k, v in batch.items()}).clone())
        return torch.cat(rows)

    try:
        assert eng._invariant_on is False
        pol.reset()
        lit = pol.select_action(batch).clone()
        lit1 = one_at_a_time(2)
        assert eng._invariant_on is False                       # literal mode: the small-batch forms stay
        bb.splice_image_tokens = True
        pol.reset()
        full = pol.select_action(batch).clone()
        alone = one_at_a_time(4)
        torch.cuda.synchronize()
        assert eng._invariant_on is True                        # ... and follow the mode
        r = max(rel_l2(alone[i:i + 1].cpu(), full[i:i + 1].cpu()) for i in range(4))
        print(f"[splice, defaults] one observation vs its row of a B = 8 call: worst row rel_l2 {r:.2e}; literal: {rel_l2(lit1.cpu(), lit[:2].cpu()):.2e}")
        assert r <= 2e-3
        assert rel_l2(lit1.cpu(), lit[:2].cpu()) <= 1e-4
        assert not torch.equal(full, lit)
        bb.splice_image_tokens = False
        pol.reset()
        pol.select_action(batch)
        assert eng._invariant_on is False
    finally:
        bb.splice_image_tokens = False
        eng.close()


# ------------------------------------------------------------------------------------------------ round 3
UNIT_TOL = 4e-3   # the op-level bound of tests/test_gpu_ops.py: one unit, bf16 output, fp32 oracle on the SAME input


def test_full_size_tower_every_unit_teacher_forced(full):
    """the per-stage test bounds the engine by the precision policy's own amplified noise (2.7e-2 at the deep
    taps).  Here each of the 51 units is compared on its own: input = what the ENGINE fed that unit (bf16 map of the previous
    unit), reference = the fp32 oracle unit on exactly that input (reference call site fastvlm_adapter.py:533; oracle
    oracle/fastvit_hd.py unit_forward, parity-unpinned).  A subtle error in any single block now shows at 4e-3, not 2.7e-2."""
    m, w, eng = full
    tc, _ = _cfgs(m)
    torch.manual_seed(31)
    img = torch.rand(1, 3, 336, 336)
    pix = eng.preprocess(img.to(DEV))
    tok, tout, taps = eng.vision_forward_unit_taps(pix)
    torch.cuda.synchronize()
    units = fastvit_hd.tower_units(tc)
    info = eng.tower_units()
    assert len(units) == len(info) == len(taps) == 1 + sum(m.tower.layers) + len(m.tower.attn_stages) + len(m.tower.layers) - 1
    assert [u[0] for u in units] == [k for k, _, _, _ in info] and [u[1] for u in units] == [st for _, st, _, _ in info]
    q = fastvit_hd.strip_prefix(w)
    x = pix.float().cpu()[..., :3].permute(0, 3, 1, 2).contiguous()
    worst = (0.0, None)
    for n, unit in enumerate(units):
        with torch.no_grad():
            ref = fastvit_hd.unit_forward(q, x, unit, tc).permute(0, 2, 3, 1)
        got = taps[n].float().cpu()
        assert got.shape == ref.shape and torch.isfinite(got).all(), (n, unit)
        r = rel_l2(got, ref)
        worst = max(worst, (r, (n, unit)))
        assert r <= UNIT_TOL, f"unit {n} {unit}: rel_l2 {r:.3e} against the fp32 oracle unit on the engine's own input"
        x = got.permute(0, 3, 1, 2).contiguous()   # teacher forcing: the next unit sees the ENGINE's output
    with torch.no_grad():
        emb = fastvit_hd.tower_head_forward(q, x, tc)
        r_emb = rel_l2(tout.float().cpu(), emb)
        r_tok = rel_l2(tok.cpu(), fastvit_hd.projector_forward(w, tout.float().cpu()))
    print(f"[fastvlm-0.5b 1024^2] 51 units teacher-forced: worst rel_l2 {worst[0]:.2e} at {worst[1]}; conv_exp+SE {r_emb:.2e}; projector {r_tok:.2e}")
    assert r_emb <= UNIT_TOL and r_tok <= UNIT_TOL


def test_c2_batch64_rows_match_batch4_and_replays_are_bit_identical(fullp):
    """BASELINE.json configs[1] (C2) at ITS batch: B=64, 336^2 -> 1024^2, 64-token prompts (the bench shape; 9.7 GB of tower
    activations, 32-bit buffer offsets and persistent-loop trip counts at their largest).  Size-independent properties: rows 0-3
    of the 64-batch equal the same four samples run as a B=4 batch (the shape the oracle checks above), two replays are
    bit-identical, and the literal-mode actions AND pooled features of ALL 64 rows meet north_star's 1e-3 against the fp32 oracle ROW BY
    ROW (the worst row, not the batch's rel-L2), under both decoder policies (VERDICT r3 #1-i)."""
    m, w, eng = fullp
    tc, lc = _cfgs(m)
    torch.manual_seed(41)
    B, T = 64, 64
    img = torch.rand(B, 3, 336, 336, device=DEV)
    ids = torch.randint(0, 151643, (B, T))
    lens = torch.full((B,), T)
    lens[1], lens[37] = 23, 1
    states = torch.randn(B, 14)
    p = _head_params(lc, 42)
    flat = _flat_head(eng, p)
    pix = eng.preprocess(img)
    tok64 = eng.vision_forward(pix)
    tok64b = eng.vision_forward(pix)
    tok4 = eng.vision_forward(pix[:4].contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(tok64).all() and torch.equal(tok64, tok64b)
    rt = rel_l2(tok64[:4].cpu(), tok4.cpu())
    rlast = rel_l2(tok64[60:].cpu(), eng.vision_forward(pix[60:].contiguous()).cpu())   # the rows with the largest offsets
    outs = []
    for _ in range(2):
        pooled = eng.backbone(img, ids, lens)
        act, _ = eng.head_forward(flat, pooled, states.to(DEV))
        torch.cuda.synchronize()
        outs.append((pooled.clone(), act.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    pooled4 = eng.backbone(img[:4].contiguous(), ids[:4], lens[:4])
    act4, _ = eng.head_forward(flat, pooled4, states[:4].to(DEV))
    torch.cuda.synchronize()
    rp = rel_l2(outs[0][0][:4].cpu(), pooled4.cpu())
    mask = (torch.arange(T)[None, :] < lens[:, None]).long()
    with torch.no_grad():   # literal mode: the decoder alone decides the feature (the tower's output is dropped)
        ref_pooled = qwen2.llm_pooled(w, ids, mask, lc)
        ref = head.head_forward(p, ref_pooled, states)
    got_p, got_a = outs[0][0].cpu(), outs[0][1].cpu()
    ra, rpo = rel_l2(got_a, ref), rel_l2(got_p, ref_pooled)
    wa, wp = worst_row(got_a, ref), worst_row(got_p, ref_pooled)
    print(f"[C2 B=64 llm_precision={eng.llm_precision}] tokens rows 0-3 vs B=4 run {rt:.2e}, rows 60-63 vs alone {rlast:.2e}; pooled rows 0-3 vs B=4 {rp:.2e}; "
          f"all 64 rows vs fp32 oracle: actions rel_l2 {ra:.2e} WORST ROW {wa:.2e}; pooled rel_l2 {rpo:.2e} WORST ROW {wp:.2e}")
    # the rows-vs-B=4 bound: another tile shape sums K in another order; the last bits then round differently into the next GEMM's operand
    # (16 significant bits in policy 1, 11 on the MLP in policy 2)
    assert rt <= 2e-3 and rlast <= 2e-3 and rp <= {1: 2e-4, 2: 1e-3, 5: 5e-4}[eng.llm_precision]
    assert ra <= 1e-3 and rpo <= 1e-3 and wa <= WORST_ROW_TOL[eng.llm_precision] and wp <= WORST_ROW_TOL[eng.llm_precision]


def test_c3_rank_shape_train_step_with_dropout(fullp):
    """BASELINE.json configs[2] (C3) per-rank shape: B=32, 64-token prompts, ONE training step with Dropout(0.1) active
    (reference fastvla/fastvlm_with_expert.py:31-37, training/trainer.py:171-182).  The kernel's Philox keep-mask is read back
    from the saved activations and handed to the oracle, so the comparison is exact in the mask: actions, loss, gradient norm,
    all 12 gradients and the AdamW update against the fp32 oracle at north_star's 1e-3 -- under both decoder policies, worst row too."""
    m, w, eng = fullp
    tc, lc = _cfgs(m)
    torch.manual_seed(51)
    B, T, pdrop = 32, 64, 0.1
    img = torch.rand(B, 3, 336, 336)
    ids = torch.randint(0, 151643, (B, T))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[5, 40:] = 0
    states, tgt = torch.randn(B, 14), torch.randn(B, 14)
    p = _head_params(lc, 52)
    flat = _flat_head(eng, p)
    pooled = eng.backbone(img.to(DEV), ids, mask.sum(1))
    act, saved = eng.head_forward(flat, pooled, states.to(DEV), training=True, dropout_p=pdrop, seed=77, offset=3)
    loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved, dropout_p=pdrop)
    mm, vv, norm, fp = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(1, device=DEV), flat.clone()
    eng.adamw_step(fp, grads, mm, vv, 1, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, grad_norm_out=norm)
    torch.cuda.synchronize()
    hid = fus = 1024
    sizes = [B * 14, B * 14, B, B * hid, B * (lc.hidden + hid), B * fus, B * fus, B, B * fus, B * fus]   # layout of `saved` (csrc/head_kernels.hip carve)
    off = sum((s + 3) // 4 * 4 for s in sizes)
    mult = saved[off: off + B * fus].view(B, fus).cpu()
    keep = (mult > 0).float()
    assert 0.88 < float(keep.mean()) < 0.92 and torch.allclose(mult[mult > 0], torch.tensor(1 / (1 - pdrop)))
    z = {k: torch.zeros_like(v) for k, v in p.items()}
    with torch.no_grad():
        ref = policy.train_step(w, p, z, z, 1, img, states, tgt, ids, mask, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, drop_mask=keep,
                                drop_p=pdrop, image_size=m.tower.image_size, llm_cfg=lc, tower_cfg=tc, run_tower=False)
    ra = rel_l2(act.cpu(), ref["pred"])
    rl = abs(float(loss) - float(ref["loss"])) / float(ref["loss"])
    rn = abs(float(norm) - float(ref["grad_norm"])) / float(ref["grad_norm"])
    wa = worst_row(act.cpu(), ref["pred"])
    print(f"[C3 rank shape B=32, dropout 0.1, llm_precision={eng.llm_precision}] keep={float(keep.mean()):.3f} actions rel_l2={ra:.2e} worst row={wa:.2e} "
          f"loss rel={rl:.2e} grad_norm rel={rn:.2e}")
    assert ra <= 1e-3 and wa <= WORST_ROW_TOL[eng.llm_precision] and rl <= 1e-3 and rn <= 1e-3
    coef = min(1.0, 1.0 / (float(ref["grad_norm"]) + 1e-6))
    gv = eng.head_views(grads)
    for k in head.HEAD_KEYS:
        rg = ref["grads"][k] / coef
        assert float((gv[k].cpu() - rg).abs().max()) <= 2e-3 * max(1e-6, float(rg.abs().max())), k
    for k, v in eng.head_views(fp).items():
        du, dr = v.cpu() - p[k], ref["params"][k] - p[k]
        bad = float(((du - dr).abs() > 0.05 * 1e-4 + 4e-3 * dr.abs()).float().mean())
        assert bad <= max(2e-3, 1.5 / du.numel()), (k, bad)


def test_decoder_precision_budget_full_size(full):
    """VERDICT r2 #4c: the per-GEMM precision budget at full size.  Same weights, inputs and head in three engines' decoders:
    llm_precision 1 (split-bf16 operands on every projection: 2x the MFMA work), 2 (split-bf16 on qkv / o only, ONE fp16 pass for
    gate/up and down: 1.12x) and 0 (plain bf16: 1x) against the fp32 oracle -- the policy table of tests/precision_budget.py
    measured on the product.  Mode 2 must meet north_star's 1e-3 on the ACTIONS; mode 0 must not be mistaken for it."""
    m, w, eng1 = full
    tc, lc = _cfgs(m)
    torch.manual_seed(71)
    B, T = 8, 64
    ids = torch.randint(0, 151643, (B, T))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, 23:] = 0
    states, tgt = torch.randn(B, 14), torch.randn(B, 14)
    p = _head_params(lc, 72)
    with torch.no_grad():
        ref_pooled = qwen2.llm_pooled(w, ids, mask, lc)
        ref_act, cache = head.head_forward(p, ref_pooled, states, keep_cache=True)
        ref_loss, ref_grads = head.head_mse_backward(p, cache, ref_act, tgt)
    out = {}
    for prec in (1, 2, 0):
        eng = eng1 if prec == 1 else FastVLAEngine(m, state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024, max_batch=8,
                                                   max_text_tokens=64, llm_precision=prec)
        if prec != 1:
            eng.load_weights(w)
        flat = _flat_head(eng, p)
        pooled = eng.llm_pooled(ids, mask.sum(1))
        act, saved = eng.head_forward(flat, pooled, states.to(DEV))
        loss, grads = eng.head_backward(flat, act, tgt.to(DEV), saved)
        torch.cuda.synchronize()
        out[prec] = (rel_l2(pooled.cpu(), ref_pooled), rel_l2(act.cpu(), ref_act))
        if prec == 2:   # the product's default mode for this model: the C1-style quantities too (loss, all 12 gradients)
            rl = abs(float(loss) - float(ref_loss)) / float(ref_loss)
            gv = eng.head_views(grads)
            rg = max(rel_l2(gv[k].cpu(), ref_grads[k]) for k in head.HEAD_KEYS)
            print(f"[llm_precision=2] loss rel {rl:.2e}, worst gradient rel_l2 {rg:.2e}")
            assert rl <= 2e-3 and rg <= 2e-3
        if prec != 1:
            eng.close()
    print("[decoder precision budget, fastvlm-0.5b B=8 T=64] (pooled, actions) rel_l2:  " +
          "  ".join(f"llm_precision={k}: {v[0]:.2e}, {v[1]:.2e}" for k, v in out.items()))
    assert out[1][1] <= 1e-4 and out[2][1] <= 1e-3 and out[2][0] <= 1.5e-3
    assert out[0][1] > out[2][1]


def test_decoder_fp16_policy_with_outlier_channels(full):
    """VERDICT r3 #1-ii / ADVICE r3 (medium): the fp16 single-pass policy on weights that look like a REAL Qwen2 checkpoint's worst
    habits instead of N(0, 0.02): four "massive activation" hidden dims (the down_proj rows of layer 1 that write them x1000, so the
    residual stream carries values ~1e3 x the rest from there on) and a 50x RMSNorm gain on one channel of every later layer.  The
    reference loads fp32 (model/fastvlm_adapter.py:183-191), so the bar stays 1e-3 on the actions against the fp32 oracle:
      * policy 1 (split-bf16; what every real checkpoint gets by default) must hold it with margin;
      * policy 2 must stay FINITE (saturating casts), report its clamps through fp16_saturations(), and its error is printed -- whether
        it holds 1e-3 on such weights is exactly why it is opt-in for real checkpoints (arch.default_llm_precision);
      * a down_proj weight beyond the fp16 range (|w| x 16 > 65504) is REFUSED at load time under policy 2, loudly."""
    from fastvla_hip import FastVLAHipError
    m, w, eng1 = full
    _, lc = _cfgs(m)
    wo = dict(w)
    dims, ch = [7, 300, 511, 880], 123
    t = wo["model.layers.1.mlp.down_proj.weight"].clone()
    t[dims] = (t[dims] * 1000).to(torch.bfloat16).float()
    wo["model.layers.1.mlp.down_proj.weight"] = t
    for i in range(2, lc.layers):
        for nm in ("input_layernorm", "post_attention_layernorm"):
            g = wo[f"model.layers.{i}.{nm}.weight"].clone()
            g[ch] *= 50.0
            wo[f"model.layers.{i}.{nm}.weight"] = g
    torch.manual_seed(91)
    B, T = 8, 64
    ids = torch.randint(0, 151643, (B, T))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[3, 30:] = 0
    states = torch.randn(B, 14)
    p = _head_params(lc, 92)
    with torch.no_grad():
        ref_pooled = qwen2.llm_pooled(wo, ids, mask, lc)
        ref_act = head.head_forward(p, ref_pooled, states)
    assert float(ref_pooled.abs().max()) > 0 and torch.isfinite(ref_pooled).all()
    res = {}
    for prec in (1, 2):
        eng = FastVLAEngine(m, state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024, max_batch=8, max_text_tokens=64, llm_precision=prec)
        eng.load_weights(wo)
        pooled = eng.llm_pooled(ids, mask.sum(1))
        act, _ = eng.head_forward(_flat_head(eng, p), pooled, states.to(DEV))
        torch.cuda.synchronize()
        assert torch.isfinite(pooled).all() and torch.isfinite(act).all(), f"llm_precision={prec}: non-finite output on outlier weights"
        res[prec] = (rel_l2(pooled.cpu(), ref_pooled), rel_l2(act.cpu(), ref_act), worst_row(act.cpu(), ref_act), eng.fp16_saturations())
        eng.close()
    print("[outlier channels, fastvlm-0.5b B=8 T=64] (pooled rel_l2, actions rel_l2, actions worst row, fp16 clamps):  " +
          "  ".join(f"llm_precision={k}: {v[0]:.2e}, {v[1]:.2e}, {v[2]:.2e}, {v[3]}" for k, v in res.items()))
    assert res[1][1] <= 3e-4 and res[1][2] <= 5e-4 and res[1][3] == 0
    # weights outside the fp16 range: refused, not clamped
    wr = dict(wo)
    t = wr["model.layers.5.mlp.down_proj.weight"].clone()
    t[11, 17] = 4608.0          # x16 = 73728 > 65504
    wr["model.layers.5.mlp.down_proj.weight"] = t
    eng = FastVLAEngine(m, state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024, max_batch=8, max_text_tokens=64, llm_precision=2)
    with pytest.raises(FastVLAHipError, match="fp16 range") as ei:
        eng.load_weights(wr)
    assert ei.value.status == -5
    eng.close()
    eng = FastVLAEngine(m, state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024, max_batch=8, max_text_tokens=64, llm_precision=1)
    eng.load_weights(wr)        # policy 1 has no range limit
    assert torch.isfinite(eng.llm_pooled(ids, mask.sum(1))).all()
    eng.close()


def test_image_prefix_cache_full_size(full):
    """SURVEY.md 8f-1 at the real dimensions: fastvlm-0.5b, 256 image tokens in front of a 32-token prompt, B=4.  The prefix pass
    (M = 1024 rows) and the suffix pass (M = 128 rows) take other GEMM tiles than the joint 288-token prefill (M = 1152), so the
    pooled rows agree to the summation order, not bit for bit; a cached row serves its image under another prompt."""
    m, w, eng = full
    torch.manual_seed(81)
    B, T = 4, 32
    tok = eng.vision_forward(eng.preprocess(torch.rand(B, 3, 336, 336).to(DEV)))
    ids = torch.randint(0, 151643, (B, T))
    lens = torch.tensor([T, 9, T, 1])
    joint = eng.llm_pooled(ids, lens, tok)
    kv = eng.llm_prefix(tok)
    pref = eng.llm_pooled_prefixed(ids, lens, kv)
    sub = torch.tensor([3, 0])
    ids2 = torch.randint(0, 151643, (2, T))
    a = eng.llm_pooled_prefixed(ids2, lens[sub], kv[:, sub].contiguous())
    b = eng.llm_pooled(ids2, lens[sub], tok[sub].contiguous())
    torch.cuda.synchronize()
    r, r2 = rel_l2(pref.cpu(), joint.cpu()), rel_l2(a.cpu(), b.cpu())
    print(f"[prefix cache fastvlm-0.5b, Ni=256, T=32] prefixed vs joint prefill {r:.2e}; re-paired rows {r2:.2e}; cache {kv.numel() * 4 / B / 2**20:.1f} MiB per image")
    assert torch.isfinite(pref).all() and r <= 2e-4 and r2 <= 2e-4


@pytest.mark.parametrize("kind", ["f32", "u8", "gray-odd-shape"])
def test_fused_letterbox_stem_equals_two_call_form(full, kind):
    """fv_vision_forward_images = fv_preprocess + fv_vision_forward with the letterbox folded into the stem kernel (the
    1024^2 frame never reaches HBM; reference: the CPU resize + H2D of model/fastvlm_adapter.py:479-488 ahead of the VLM call at :533).
    The stem samples the source image with letterbox_kernel's own arithmetic, so the image tokens must be BIT-identical -- for float and
    uint8 sources, RGB and gray, square and non-square (left / top padding, fastvlm_adapter.py:36-55)."""
    m, w, eng = full
    g = torch.Generator().manual_seed(91)
    if kind == "f32":
        img = torch.rand(3, 3, 336, 336, generator=g)
    elif kind == "u8":
        img = torch.randint(0, 256, (2, 3, 336, 336), generator=g, dtype=torch.uint8)
    else:
        img = torch.rand(2, 1, 210, 333, generator=g)
    img = img.to(DEV)
    a, ta = eng.vision_forward(eng.preprocess(img, pad_value=0.25), return_tower_out=True)
    b, tb = eng.vision_forward_images(img, pad_value=0.25, return_tower_out=True)
    torch.cuda.synchronize()
    assert torch.isfinite(b).all() and torch.equal(ta, tb) and torch.equal(a, b)
