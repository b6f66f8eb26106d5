"""Prompt reuse (fv_set_prompt_reuse): in literal mode the engine keeps the pooled rows of the last prompt on the device and returns them while the key
(ids up to lens, lens, B, T, pool_mode) stays the same.  Every claim here is bit-for-bit (torch.equal): a hit must be what a recomputation gives, and a miss
must be what an engine with reuse off gives.  Shapes: the "tiny" preset (the smallest the GPU tests use; head_dim 32) for the literal call itself, "small"
(head_dim 64) where fv_train_begin / the prefixed call need it; B <= 4, T <= 16."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV  # noqa: E402
from fastvla_hip import FastVLAEngine, FastVLAHipError, arch, lora, weights  # noqa: E402

B, T = 3, 12
_W = {}


def _weights(preset, seed=5):
    if (preset, seed) not in _W:
        _W[(preset, seed)] = weights.init_backbone(arch.preset(preset), seed=seed)
    return _W[(preset, seed)]


def _engine(preset="tiny", reuse=True, seed=5, precision=1, load=True):
    eng = FastVLAEngine(arch.preset(preset), state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64, max_batch=4, max_text_tokens=16, llm_precision=precision)
    if load:
        eng.load_weights(_weights(preset, seed))
    if not reuse:
        eng.set_prompt_reuse(False)
    return eng


def _prompt(preset="tiny", b=B, t=T, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, arch.preset(preset).llm.vocab, (b, t), generator=g).to(DEV, torch.int32)
    lens = torch.tensor([t, max(t // 2, 1), 1, t - 1][:b]).to(DEV, torch.int32)
    return ids, lens


def _pooled(eng, ids, lens, pool_mode=0):
    out = eng.llm_pooled(ids, lens, None, pool_mode).clone()
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def ref_tiny():
    """ONE engine with reuse off: the recomputation every miss and every hit is compared with"""
    eng = _engine(reuse=False)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 1, 5: hit, first call, switch
@pytest.mark.parametrize("precision", [0, 1])
def test_second_identical_call_hits_and_is_bit_equal(precision):
    eng = _engine(precision=precision)
    ids, lens = _prompt()
    assert eng.prompt_reuse_stats() == (0, 0)
    a = _pooled(eng, ids, lens)
    assert eng.prompt_reuse_stats() == (1, 0)        # 5. the first call after construction misses: `valid` starts clear
    b = _pooled(eng, ids, lens)
    assert eng.prompt_reuse_stats() == (2, 1)
    assert torch.equal(a, b) and torch.isfinite(a).all() and float(a.abs().max()) > 0
    off = _engine(reuse=False, precision=precision)
    c, d = _pooled(off, ids, lens), _pooled(off, ids, lens)
    assert off.prompt_reuse_stats() == (0, 0)        # reuse off: the slot is never touched
    assert torch.equal(c, d) and torch.equal(a, c)
    eng.set_prompt_reuse(False)
    assert torch.equal(_pooled(eng, ids, lens), a) and eng.prompt_reuse_stats() == (2, 1)
    eng.set_prompt_reuse(True)                       # switching back on re-proves the slot: one miss, then hits
    assert torch.equal(_pooled(eng, ids, lens), a) and eng.prompt_reuse_stats() == (3, 1)
    assert torch.equal(_pooled(eng, ids, lens), a) and eng.prompt_reuse_stats() == (4, 2)
    eng.close()
    off.close()


def test_hit_overwrites_the_callers_buffer(ref_tiny):
    """the hit path writes the caller's pooled rows itself (llm_pooled hands out a fresh torch.empty buffer; poison what the allocator may hand back)"""
    eng = _engine()
    ids, lens = _prompt()
    a = _pooled(eng, ids, lens)
    junk = [torch.full((B, arch.preset("tiny").llm.hidden), float("nan"), device=DEV) for _ in range(4)]
    del junk
    b = _pooled(eng, ids, lens)
    assert eng.prompt_reuse_stats() == (2, 1) and torch.equal(a, b) and torch.equal(a, _pooled(ref_tiny, ids, lens))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2, 3, 6: the key
def _changed(case):
    """-> (ids, lens, pool_mode) of the second call"""
    ids, lens = _prompt()
    ids, lens = ids.clone(), lens.clone()
    if case == "token":
        ids[1, 2] = (ids[1, 2] + 1) % arch.preset("tiny").llm.vocab      # row 1 has lens = T / 2 = 6: position 2 is inside
    elif case == "last-valid-token":
        ids[1, T // 2 - 1] = (ids[1, T // 2 - 1] + 1) % arch.preset("tiny").llm.vocab
    elif case == "first-token-of-a-one-token-row":
        ids[2, 0] = (ids[2, 0] + 1) % arch.preset("tiny").llm.vocab      # row 2 has lens = 1
    elif case == "lens":
        lens[1] += 1
    elif case == "B":
        ids, lens = ids[:2].contiguous(), lens[:2].contiguous()
    elif case == "T":
        ids, lens = ids[:, :T - 1].contiguous(), lens.clamp(max=T - 1)
    return ids, lens, 1 if case == "pool_mode" else 0


@pytest.mark.parametrize("case", ["token", "last-valid-token", "first-token-of-a-one-token-row", "lens", "B", "T", "pool_mode"])
def test_changed_key_misses_and_matches_recomputation(case, ref_tiny):
    eng = _engine()
    ids0, lens0 = _prompt()
    first = _pooled(eng, ids0, lens0)
    assert torch.equal(_pooled(eng, ids0, lens0), first) and eng.prompt_reuse_stats() == (2, 1)
    ids, lens, mode = _changed(case)
    got = _pooled(eng, ids, lens, mode)
    assert eng.prompt_reuse_stats() == (3, 1), case                     # a miss
    assert torch.equal(got, _pooled(ref_tiny, ids, lens, mode)), case
    if case not in ("B", "T"):
        assert not torch.equal(got, first), case                        # (the change is one the result can see)
    assert torch.equal(_pooled(eng, ids, lens, mode), got) and eng.prompt_reuse_stats() == (4, 2)   # the slot now holds the new key
    assert torch.equal(_pooled(eng, ids0, lens0), first) and eng.prompt_reuse_stats() == (5, 2)     # ... and no longer the old one
    eng.close()


def test_padding_ids_are_not_part_of_the_key(ref_tiny):
    """3. ids at positions >= lens[b] cannot reach pooled (causal attention with keys >= lens masked, row-wise kernels, pooling over rows < lens): the probe
    compares the valid prefix only, so a changed padding id hits -- and the kept rows are what an engine with reuse off computes from the CHANGED ids."""
    eng = _engine()
    ids, lens = _prompt()
    a = _pooled(eng, ids, lens)
    pad = ids.clone()
    pad[1, T // 2:] = (pad[1, T // 2:] + 7) % arch.preset("tiny").llm.vocab     # row 1: every position from lens[1] on
    pad[2, 1:] = 0                                                               # row 2 (lens = 1): everything behind its one token
    for mode in (0, 1):
        assert torch.equal(_pooled(ref_tiny, pad, lens, mode), _pooled(ref_tiny, ids, lens, mode)), mode   # the masking assumption itself
    b = _pooled(eng, pad, lens)
    assert eng.prompt_reuse_stats() == (2, 1)
    assert torch.equal(a, b) and torch.equal(b, _pooled(ref_tiny, pad, lens))
    eng.close()


def test_one_slot_b2_b4_b2(ref_tiny):
    """6. B = 2, then B = 4 with the same leading rows, then B = 2 again: three misses (the single slot holds the last key)"""
    eng = _engine()
    ids4, lens4 = _prompt(b=4)
    ids2, lens2 = ids4[:2].contiguous(), lens4[:2].contiguous()
    a2 = _pooled(eng, ids2, lens2)
    a4 = _pooled(eng, ids4, lens4)
    b2 = _pooled(eng, ids2, lens2)
    assert eng.prompt_reuse_stats() == (3, 0)
    assert torch.equal(a2, _pooled(ref_tiny, ids2, lens2)) and torch.equal(a4, _pooled(ref_tiny, ids4, lens4)) and torch.equal(b2, a2)
    assert torch.equal(_pooled(eng, ids2, lens2), a2) and eng.prompt_reuse_stats() == (4, 1)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4: invalidation
def _train_pair():
    """two "small" engines (head_dim 64: fv_train_begin's floor) in training state, reuse on / off, and the exported master"""
    eng, off = _engine("small"), _engine("small", reuse=False)
    flats = []
    for e in (eng, off):
        e.train_begin()
        _, total, _ = e.train_layout()
        flat = torch.zeros(total, device=DEV)
        e.train_export_params(flat)
        flats.append(flat)
    assert torch.equal(flats[0], flats[1])
    return eng, off, flats[0]


def _warm(eng, ids, lens):
    """a miss and a hit -> (pooled, (calls, hits))"""
    a = _pooled(eng, ids, lens)
    assert torch.equal(_pooled(eng, ids, lens), a)
    return a, eng.prompt_reuse_stats()


def _expect_miss(eng, off, ids, lens, stats, what):
    got = _pooled(eng, ids, lens)
    assert eng.prompt_reuse_stats() == (stats[0] + 1, stats[1]), what          # a miss ...
    assert torch.equal(got, _pooled(off, ids, lens)), what                      # ... that is the recomputation
    assert torch.equal(_pooled(eng, ids, lens), got) and eng.prompt_reuse_stats() == (stats[0] + 2, stats[1] + 1), what
    return got, eng.prompt_reuse_stats()


def test_weights_load_once_and_the_first_call_misses():
    """fv_load_weights / fv_load_weights_cb: a handle takes its weights ONCE (a second load is FV_ERR_STATE), so "the same prompt after a load with other weights"
    is a first call on another handle: it misses, and two handles with different weights never share a slot"""
    ids, lens = _prompt()
    e1, e2 = _engine(seed=5), _engine(seed=6)
    with pytest.raises(FastVLAHipError):
        e1.load_weights(_weights("tiny", 6))
    a1, a2 = _pooled(e1, ids, lens), _pooled(e2, ids, lens)
    assert e1.prompt_reuse_stats() == (1, 0) and e2.prompt_reuse_stats() == (1, 0)
    assert not torch.equal(a1, a2)
    off = _engine(seed=6, reuse=False)
    assert torch.equal(a2, _pooled(off, ids, lens))
    for e in (e1, e2, off):
        e.close()


def test_train_commit_and_option_switches_invalidate():
    eng, off, flat = _train_pair()
    ids, lens = _prompt("small")
    base, st = _warm(eng, ids, lens)
    g = torch.Generator().manual_seed(3)
    pert = flat + 0.05 * torch.randn(flat.shape, generator=g).to(DEV) * flat.abs().clamp_min(1e-3)
    for e in (eng, off):
        e.train_commit(pert)
    got, st = _expect_miss(eng, off, ids, lens, st, "fv_train_commit")
    assert not torch.equal(got, base)
    for e in (eng, off):
        e.train_set_options(grad_split=1)
    _, st = _expect_miss(eng, off, ids, lens, st, "fv_train_set_options")
    for e in (eng, off):
        e.train_set_forward_f16(True)
    _, st = _expect_miss(eng, off, ids, lens, st, "fv_train_set_forward_f16")
    for e in (eng, off):
        e.set_batch_invariant(True)
    _, st = _expect_miss(eng, off, ids, lens, st, "fv_set_batch_invariant")
    eng.close()
    off.close()


@pytest.mark.parametrize("dora", [False, True])
def test_lora_commit_merge_and_magnitude_invalidate(dora):
    eng, off, flat = _train_pair()
    ids, lens = _prompt("small")
    base, st = _warm(eng, ids, lens)
    lflats = []
    for e in (eng, off):
        e.train_lora_begin(4, 8.0, dora=dora)
        lt, ltotal = e.train_lora_layout()
        lflat = torch.zeros(ltotal, device=DEV)
        lflat[:lt[16]["offset"]].copy_(flat[:lt[16]["offset"]])
        lora.init_adapters(lflat, lt, seed=1)
        gB = torch.Generator().manual_seed(9)
        for name, v in lora.adapter_views(lflat, lt).items():
            if name.endswith(".lora_B.weight"):
                v.copy_((torch.randn(v.shape, generator=gB) * 0.05).to(DEV))
        lflats.append(lflat)
    if dora:
        for e, lf in zip((eng, off), lflats):
            e.train_lora_init_magnitude(flat, lf)
        _, st = _expect_miss(eng, off, ids, lens, st, "fv_train_lora_init_magnitude")
    for e, lf in zip((eng, off), lflats):
        e.train_lora_commit(flat, lf)
    got, st = _expect_miss(eng, off, ids, lens, st, "fv_train_lora_commit")
    assert not torch.equal(got, base)
    for e, lf in zip((eng, off), lflats):
        e.train_lora_merge(flat.clone(), lf)
    _, st = _expect_miss(eng, off, ids, lens, st, "fv_train_lora_merge")
    eng.close()
    off.close()


# ------------------------------------------------------------------------------------------------------------------ 7: hipGraph
def test_captured_step_decides_on_every_replay():
    m = arch.preset("tiny")
    eng, off = _engine(), _engine(reuse=False)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 96, 96, generator=g).to(DEV)
    states = torch.randn(2, 14, generator=g).to(DEV)
    flat = (torch.randn(eng.head_numel(), generator=g) * 0.1).to(DEV)
    ids, lens = _prompt(b=2)
    ids_new = ids.clone()
    ids_new[0, 0] = (ids_new[0, 0] + 1) % m.llm.vocab

    def eager(e, i):
        act, _ = e.head_forward(flat, e.backbone(images, i, lens), states)
        torch.cuda.synchronize()
        return act.clone()

    ref_old, ref_new = eager(off, ids), eager(off, ids_new)
    assert not torch.equal(ref_old, ref_new)
    static_ids = ids.clone()
    replay, actions = eng.capture_policy_step(images, static_ids, lens, flat, states)
    c0, h0 = eng.prompt_reuse_stats()
    replay(); torch.cuda.synchronize()
    a1 = actions.clone()
    replay(); torch.cuda.synchronize()
    a2 = actions.clone()
    c1, h1 = eng.prompt_reuse_stats()
    assert (c1 - c0, h1 - h0) == (2, 2)                 # the warm-up steps left the slot holding these ids: both replays hit
    print(f"[capture] replay 1 vs 2 max |diff| {float((a1 - a2).abs().max()):.3e}; replay 1 vs eager reuse-off {float((a1 - ref_old).abs().max()):.3e}")
    assert torch.equal(a1, a2)
    assert torch.equal(a1, ref_old)
    static_ids.copy_(ids_new)
    replay(); torch.cuda.synchronize()
    a3 = actions.clone()
    assert eng.prompt_reuse_stats() == (c1 + 1, h1)    # the same graph, new ids: a miss, decided on the device
    assert torch.equal(a3, ref_new)
    replay(); torch.cuda.synchronize()
    assert eng.prompt_reuse_stats() == (c1 + 2, h1 + 1) and torch.equal(actions, ref_new)
    eng.close()
    off.close()


# ------------------------------------------------------------------------------------------------------------------ 8: the other decoder calls
def test_splice_and_prefixed_calls_leave_the_slot_alone():
    m = arch.preset("small")
    eng, off = _engine("small"), _engine("small", reuse=False)
    ids, lens = _prompt("small")
    g = torch.Generator().manual_seed(2)
    tok = (torch.randn(B, m.tower.num_tokens, m.llm.hidden, generator=g) * 0.5).to(DEV)
    base, st = _warm(eng, ids, lens)
    s1 = eng.llm_pooled(ids, lens, tok).clone()
    s2 = eng.llm_pooled(ids, lens, tok).clone()
    kv = eng.llm_prefix(tok)
    p1 = eng.llm_pooled_prefixed(ids, lens, kv).clone()
    p2 = eng.llm_pooled_prefixed(ids, lens, kv).clone()
    torch.cuda.synchronize()
    assert eng.prompt_reuse_stats() == st
    assert torch.equal(s1, s2) and torch.equal(p1, p2) and not torch.equal(s1, base)
    assert torch.equal(s1, off.llm_pooled(ids, lens, tok)) and torch.equal(p1, off.llm_pooled_prefixed(ids, lens, off.llm_prefix(tok)))
    assert torch.equal(_pooled(eng, ids, lens), base) and eng.prompt_reuse_stats() == (st[0] + 1, st[1] + 1)   # the slot survived them
    eng.close()
    off.close()


# ------------------------------------------------------------------------------------------------------------------ 9: the profiler
def test_profile_counts_executed_work_only():
    eng, off = _engine(), _engine(reuse=False)
    ids, lens = _prompt()
    off.profile(True)
    _pooled(off, ids, lens)
    one, one_shapes = off.profile_read()
    off.profile(False)
    eng.profile(True)
    _pooled(eng, ids, lens)     # miss
    _pooled(eng, ids, lens)     # hit
    assert eng.prompt_reuse_stats() == (2, 1)
    two, two_shapes = eng.profile_read()
    eng.profile(False)
    assert one["gemm"]["flops"] > 0 and one["attention"]["flops"] > 0
    for fam in ("gemm", "attention", "norm"):
        assert two[fam]["flops"] == one[fam]["flops"] and two[fam]["bytes"] == one[fam]["bytes"], fam     # exactly ONE call's decoder work
        assert two[fam]["launches"] == 2 * one[fam]["launches"], fam                                        # ... and both calls' launches
    key = lambda r: (r["m"], r["n"], r["k"], r["epi"])
    assert {key(r): r["launches"] for r in two_shapes} == {key(r): r["launches"] for r in one_shapes}
    eng.close()
    off.close()
