"""-m gpu: several samples per observation from the flow head, one chosen on the device (fv_head_set_flow_samples / fv_head_flow_sample_multi).

1. Identity (torch.equal): candidate s of a call at offset o is the single-sample call at o + (s << 56) -- plain and prefix sampler, drawn and explicit noise,
   Euler and RK4, folded statistics off and on; "first" serves the single call's actions; S = 1 is a handle that never called the setter; two calls agree.
2. The selection kernel alone (fv_op_flow_select) on candidates the test supplies: exact cases (small integers: every fp32 sum is exact, scores equal the
   float64 values and the choice the reference's), NaN / inf cases, and random cases.
   Bar of the random cases: scores and spread within 4 x the fp32 CPU emulation's distance from float64 (flow_samples_util.emulation_distance, one figure per
   head and score; tests/test_flow_samples_host.py keeps it below 1e-5), the project's sampler bar.  The choice must equal the float64 argmin on every row
   whose float64 runner-up lies more than that bar above the winner; closer rows are left out, at most 5 % of all rows of all cases (the host test checks
   the cap on the reference alone; the two-candidate medoid, an exact tie by construction, must choose candidate 0 and does not count).  chunk_out is bitwise the chosen candidate, actions its single fused multiply-add."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_prefix_util as pu  # noqa: E402
import flow_samples_util as sm  # noqa: E402
import flow_solver_util as su  # noqa: E402
import flow_util as fu  # noqa: E402
from gpu_util import DEV, lib, stream  # noqa: E402
from fastvla_hip import FastVLAEngine, _lib, arch  # noqa: E402
from fastvla_hip.select import coherence_weights  # noqa: E402

SEED, OFFSET = 4321, (5 << 40) + 9
SAMPLES = (1, 2, 5, 16)


def _engine(name, B, *, samples=None, weights=None, solver=None, D=None):
    """a head-only engine in flow mode.  samples None: the handle never calls the setter"""
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=ds, action_dim=K * A, hidden_dim=hid, fusion_dim=fus, max_batch=B)
    eng.set_head_flow(E)
    if D is not None:
        eng.set_head_flow_prefix(K, D)
    if solver is not None:
        eng.set_head_flow_solver(solver)
    if samples is not None:
        eng.set_head_flow_samples(samples, weights)
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


def _off(s):
    return OFFSET + (s << 56)


# ------------------------------------------------------------------------------------------------------------------ 1. identity
def _plain_identity(name, B, solver, samples, steps):
    c = fu.sampler_case(name, B)
    da = c["dims"][4] * c["dims"][5]
    eng = _engine(name, B, samples=16, solver=solver)
    flat = _flat(eng, c["p"])
    pooled, states = c["pooled"].to(DEV), c["states"].to(DEV)
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(16 * B, da, generator=g).to(DEV)
    for io in (False, True):
        _set_io(eng, c["stats"], io)
        for N in steps:
            single = [eng.head_flow_sample(flat, pooled, states, steps=N, seed=SEED, offset=_off(s)) for s in range(max(samples))]
            single_n = [eng.head_flow_sample(flat, pooled, states, steps=N, noise=noise[s * B:(s + 1) * B]) for s in range(max(samples))]
            for S in samples:
                out = eng.head_flow_sample_multi(flat, pooled, states, samples=S, select="first", steps=N, seed=SEED, offset=OFFSET)
                again = eng.head_flow_sample_multi(flat, pooled, states, samples=S, select="first", steps=N, seed=SEED, offset=OFFSET)
                outn = eng.head_flow_sample_multi(flat, pooled, states, samples=S, select="first", steps=N, noise=noise[:S * B])
                tag = (name, B, solver, io, N, S)
                assert all(torch.equal(out[k], again[k]) for k in out), tag                       # two calls agree
                assert torch.equal(out["actions"], single[0]) and torch.equal(outn["actions"], single_n[0]), tag      # "first" is the single call
                assert torch.equal(out["chunk"], out["candidates"][:B]) and bool((out["choice"] == 0).all()), tag
                for s in range(S):
                    rows, rows_n = out["candidates"][s * B:(s + 1) * B], outn["candidates"][s * B:(s + 1) * B]
                    if not io:      # no folded statistics: the single call returns the normalised chunk itself
                        assert torch.equal(rows, single[s]) and torch.equal(rows_n, single_n[s]), (tag, s)
                    else:           # folded: the one-candidate call at the candidate's offset ties the normalised row to the single call's actions
                        one = eng.head_flow_sample_multi(flat, pooled, states, samples=1, select="first", steps=N, seed=SEED, offset=_off(s))
                        assert torch.equal(one["actions"], single[s]) and torch.equal(one["chunk"], rows), (tag, s)
    torch.cuda.synchronize()
    eng.close()


@pytest.mark.parametrize("solver", ("euler", "rk4"))
@pytest.mark.parametrize("B", (1, 9))
@pytest.mark.parametrize("name", ("awkward", "larger"))
def test_candidates_are_the_single_sample_calls(name, B, solver):
    _plain_identity(name, B, solver, SAMPLES, (1, 4))


def test_candidates_are_the_single_sample_calls_many_rows():
    _plain_identity("awkward", 67, "euler", (3,), (4,))


@pytest.mark.parametrize("solver", ("euler", "rk4"))
@pytest.mark.parametrize("B", (1, 9))
@pytest.mark.parametrize("name", ("awkward", "larger"))
def test_prefix_candidates_are_the_prefix_sampler_calls_and_keep_the_pinned_bits(name, B, solver):
    c = su.prefix_case(name, B)
    K, A, D = c["dims"][4], c["dims"][5], c["D"]
    da = K * A
    eng = _engine(name, B, samples=16, solver=solver, D=D)
    flat = _flat(eng, c["p"])
    pooled, states, prev, delays = c["pooled"].to(DEV), c["states"].to(DEV), c["prev"].to(DEV), torch.from_numpy(c["delays"]).to(DEV)
    noise = torch.randn(16 * B, da, generator=torch.Generator().manual_seed(6)).to(DEV)
    for shift in (0, K // 3):
        pin = pu.pinned_steps(c["delays"], D, K, shift)
        pinned = torch.from_numpy(pu.mask_ref(pin, K)).bool().repeat_interleave(A, dim=1).to(DEV)
        src = torch.zeros(B, da, device=DEV)
        src[:, :da - shift * A] = prev[:, shift * A:]
        for io in (False, True):
            _set_io(eng, c["stats"], io)
            for N in (1, 4):
                for S in SAMPLES:
                    out = eng.head_flow_sample_multi(flat, pooled, states, samples=S, select="first", prev=prev, shift=shift, delays=delays, steps=N, seed=SEED, offset=OFFSET)
                    outn = eng.head_flow_sample_multi(flat, pooled, states, samples=S, select="first", prev=prev, shift=shift, delays=delays, steps=N, noise=noise[:S * B])
                    for s in range(S):
                        act, chunk = eng.head_flow_sample_prefix(flat, pooled, states, prev, delays, shift=shift, steps=N, seed=SEED, offset=_off(s))
                        _, chunk_n = eng.head_flow_sample_prefix(flat, pooled, states, prev, delays, shift=shift, steps=N, noise=noise[s * B:(s + 1) * B])
                        rows, rows_n = out["candidates"][s * B:(s + 1) * B], outn["candidates"][s * B:(s + 1) * B]
                        tag = (name, B, solver, shift, io, N, S, s)
                        assert torch.equal(rows, chunk) and torch.equal(rows_n, chunk_n), tag
                        assert torch.equal(rows[pinned], src[pinned]) and torch.equal(rows_n[pinned], src[pinned]), tag      # prev's bits in every candidate
                        if s == 0:
                            assert torch.equal(out["actions"], act), tag
    torch.cuda.synchronize()
    eng.close()


def test_one_sample_is_a_handle_that_never_called_the_setter_and_refusals():
    name, B = "awkward", 9
    c = fu.sampler_case(name, B)
    K = c["dims"][4]
    fresh, eng = _engine(name, B), _engine(name, B, samples=4)
    pooled, states = c["pooled"].to(DEV), c["states"].to(DEV)
    ff, fe = _flat(fresh, c["p"]), _flat(eng, c["p"])
    for io in (False, True):
        _set_io(fresh, c["stats"], io), _set_io(eng, c["stats"], io)
        ref = fresh.head_flow_sample(ff, pooled, states, steps=4, seed=SEED, offset=OFFSET)
        a = fresh.head_flow_sample_multi(ff, pooled, states, samples=1, steps=4, seed=SEED, offset=OFFSET)
        b = eng.head_flow_sample_multi(fe, pooled, states, samples=1, steps=4, seed=SEED, offset=OFFSET)
        assert torch.equal(a["actions"], ref) and torch.equal(b["actions"], ref) and torch.equal(a["chunk"], b["chunk"])
        bare = fresh.head_flow_sample_multi(ff, pooled, states, samples=1, steps=4, seed=SEED, offset=OFFSET, extras=False)      # no optional output: no selection launch
        assert set(bare) == {"actions", "chunk"} and torch.equal(bare["actions"], ref) and torch.equal(bare["chunk"], a["chunk"])
        assert torch.equal(eng.head_flow_sample(fe, pooled, states, steps=4, seed=SEED, offset=OFFSET), ref)      # the plain call on a grown plan
        assert float(a["spread"].abs().max()) == 0.0 and float(a["scores"].abs().max()) == 0.0
    assert fresh.workspace_bytes(B, 1, False) < eng.workspace_bytes(B, 1, False)
    kw = dict(steps=2, seed=SEED)
    with pytest.raises(RuntimeError, match="max_samples"):
        fresh.head_flow_sample_multi(ff, pooled, states, samples=2, **kw)
    with pytest.raises(RuntimeError, match="max_samples"):
        eng.head_flow_sample_multi(fe, pooled, states, samples=5, **kw)
    with pytest.raises(RuntimeError, match="step weights"):
        eng.head_flow_sample_multi(fe, pooled, states, samples=2, select="coherent", prev=c["noise"], **kw)
    with pytest.raises(RuntimeError, match="bits 56"):
        eng.head_flow_sample_multi(fe, pooled, states, samples=2, offset=1 << 57, **kw)
    with pytest.raises(RuntimeError, match="prefix mode"):
        eng.head_flow_sample_multi(fe, pooled, states, samples=2, prev=c["noise"], delays=torch.zeros(B, dtype=torch.int32), **kw)
    with pytest.raises(RuntimeError, match="before fv_bind_workspace"):
        eng.set_head_flow_samples(8)
    with pytest.raises(ValueError, match="flow_samples"):
        eng.set_head_flow_samples(17)
    with pytest.raises(RuntimeError, match="outside 1"):
        _lib.check(eng.lib.fv_head_set_flow_samples(eng.h, 17, 0, None), "fv_head_set_flow_samples", eng.h)
    eng.set_head_flow_samples(4, coherence_weights(K, 0.5))              # same count, weights now: allowed after the workspace is bound
    out = eng.head_flow_sample_multi(fe, pooled, states, samples=2, select="coherent", prev=c["noise"], shift=1, **kw)
    with pytest.raises(RuntimeError, match="shift"):
        eng.head_flow_sample_multi(fe, pooled, states, samples=2, select="coherent", prev=c["noise"], shift=K + 1, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["actions"]).all())
    fresh.close(), eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the selection kernel alone
def _op_select(c, select, *, cand=None, prev=None, shift=None, masked=True, io=True):
    """fv_op_flow_select on case c -> dict of numpy arrays; cand / prev replace the case's"""
    cand = c["cand"] if cand is None else cand
    S, B, da = cand.shape
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    x, pv, w, mask = d(cand.reshape(S * B, da)), d(c["prev"] if prev is None else prev), d(c["w"]), d(c["row_mask"] if masked else None)
    std, mean = (d(c["std"]), d(c["mean"])) if io else (None, None)
    out = dict(actions=torch.empty(B, da, device=DEV), chunk=torch.empty(B, da, device=DEV), candidates=torch.empty(S * B, da, device=DEV),
               choice=torch.empty(B, dtype=torch.int32, device=DEV), scores=torch.empty(B, S, device=DEV), spread=torch.empty(B, da, device=DEV))
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    _lib.check(lib().fv_op_flow_select(x.data_ptr(), B, S, da, _lib.FLOW_SELECTS[select], p(pv), c["shift"] if shift is None else shift, p(mask), p(w), c["K"],
                                       p(std), p(mean), *(out[k].data_ptr() for k in ("actions", "chunk", "candidates", "choice", "scores", "spread")), stream()),
               "fv_op_flow_select")
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    # whatever the scores: chunk_out is bitwise the chosen candidate, actions its single fused multiply-add, candidates_out a copy
    chosen = cand[res["choice"], np.arange(B)]
    assert np.array_equal(res["chunk"].view(np.uint32), chosen.view(np.uint32))
    assert np.array_equal(res["candidates"].view(np.uint32), cand.reshape(S * B, da).view(np.uint32))
    if io:
        fma = (chosen.astype(np.float64) * c["std"].astype(np.float64) + c["mean"].astype(np.float64)).astype(np.float32)      # exact product, one rounding
        assert np.array_equal(res["actions"].view(np.uint32), fma.view(np.uint32))
    else:
        assert np.array_equal(res["actions"].view(np.uint32), chosen.view(np.uint32))
    return res


@pytest.mark.parametrize("S", (1, 2, 5, 16))
@pytest.mark.parametrize("B", (1, 9))
@pytest.mark.parametrize("name", ("awkward", "larger"))
def test_select_exact_cases(name, B, S):
    c = sm.exact_case(name, B, S)
    K = c["K"]
    for select in sm.SELECTS:
        for shift in (sm.SHIFTS(K) if select == "coherent" else (0,)):
            for masked in ((True, False) if select == "coherent" else (True,)):
                kw = sm.case_kwargs(c, select, shift=shift, masked=masked)
                sc, ch, _ = sm.select_ref(c["cand"], select, **kw)
                got = _op_select(c, select, shift=shift, masked=masked, io=bool(shift % 2 == 0))
                tag = (name, B, S, select, shift, masked)
                assert np.array_equal(got["scores"].astype(np.float64), sc), tag               # every sum is exact in fp32
                assert np.array_equal(got["choice"], ch), tag
                if S > 1 and not masked:
                    # candidates 0 and S - 1 are one chunk: a duplicate pair ties.  At shift 0 every other row has it for prev: both score 0, the lower wins
                    assert np.array_equal(got["scores"][:, 0], got["scores"][:, S - 1]) and bool((got["choice"] != S - 1).all()), tag
                    assert shift != 0 or bool((got["choice"][::2] == 0).all() and (got["scores"][::2, 0] == 0).all()), tag
                if select == "coherent" and shift == K:
                    assert bool((got["choice"][c["row_mask"] != 0] == 0).all()) if masked else bool((got["choice"] == 0).all()), tag
    # row_mask 0 under "coherent" gives the medoid's choice; all-zero weights choose candidate 0
    med = _op_select(c, "medoid")
    coh = _op_select(c, "coherent")
    off = c["row_mask"] == 0
    assert np.array_equal(coh["choice"][off], med["choice"][off]) and np.array_equal(coh["scores"][off], med["scores"][off])
    zero = dict(c, w=np.zeros(K, np.float32))
    assert bool((_op_select(zero, "coherent", masked=False)["choice"] == 0).all())


@pytest.mark.parametrize("name", ("awkward", "larger"))
def test_select_non_finite_candidates_never_win(name):
    B, S = 9, 5
    c = sm.exact_case(name, B, S)
    K, A = c["K"], c["A"]
    base = {sel: _op_select(c, sel, masked=False) for sel in ("medoid", "coherent")}
    for bad_value in (np.nan, np.inf, -np.inf):
        cand = c["cand"].copy()
        for b in range(B):                       # one bad candidate per row, every index in turn; one element of it, anywhere in the chunk
            cand[b % S, b, (7 * b) % (K * A)] = bad_value
        for select in ("medoid", "coherent"):
            kw = sm.case_kwargs(c, select, masked=False)
            sc, ch, _ = sm.select_ref(cand, select, **kw)
            got = _op_select(c, select, cand=cand, masked=False)
            assert np.array_equal(got["scores"].astype(np.float64), sc) and np.array_equal(got["choice"], ch), (name, bad_value, select)
            assert all(got["choice"][b] != b % S for b in range(B)), (name, bad_value, select)
            assert bool(np.isinf(got["scores"][np.arange(B), np.arange(B) % S]).all())
        # every candidate bad: candidate 0
        allbad = c["cand"].copy()
        allbad[:, :, 0] = bad_value
        for select in ("medoid", "coherent"):
            got = _op_select(c, select, cand=allbad, masked=False, io=False)
            assert bool((got["choice"] == 0).all()) and bool(np.isinf(got["scores"]).all()), (name, bad_value, select)
        # prev beyond the overlap is never read: NaN / inf there change no bit
        shift = c["shift"] if c["shift"] > 0 else 1
        prev = c["prev"].copy()
        prev[:, :shift * A] = bad_value
        ref = _op_select(c, "coherent", shift=shift, masked=False)
        got = _op_select(c, "coherent", prev=prev, shift=shift, masked=False)
        assert all(np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)) for k in got), (name, bad_value)
    assert base["medoid"]["scores"].shape == (B, S)


@pytest.mark.parametrize("name,B,S", sm.RANDOM_CASES)
def test_select_random_cases(name, B, S):
    c = sm.random_case(name, B, S)
    for select in ("medoid", "coherent"):
        kw = sm.case_kwargs(c, select)
        sc, ch, sp = sm.select_ref(c["cand"], select, **kw)
        d_sc, d_sp = sm.emulation_distance(name, select)
        got = _op_select(c, select)
        e_sc, e_sp = sm.rel_dist(got["scores"], sc), sm.rel_dist(got["spread"], sp)
        print(f"[select {select} {name} B={B} S={S}] scores {e_sc:.3e} (emulation {d_sc:.3e}), spread {e_sp:.3e} (emulation {d_sp:.3e})")
        assert e_sc <= 4 * d_sc and e_sp <= 4 * d_sp, (select, e_sc, d_sc, e_sp, d_sp)
        decided = sm.decided_rows(sc, 4 * d_sc)
        assert np.array_equal(got["choice"][decided], ch[decided]), (select, got["choice"], ch)
        if select == "medoid" and S == 2:      # two candidates are each other's only distance: an exact tie on every row, and the lower index wins
            assert bool((got["choice"] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ 3. the policy
ENV = ("FASTVLA_ACTION_HEAD", "FASTVLA_FLOW_SAMPLES", "FASTVLA_FLOW_SELECT", "FASTVLA_FLOW_COHERENCE_DECAY", "FASTVLA_FLOW_SOLVER", "FASTVLA_RTC", "FASTVLA_RTC_METHOD",
       "FASTVLA_TEMPORAL_ENSEMBLE_COEFF", "FASTVLA_FLOW_PREFIX_MAX_DELAY", "FASTVLA_FLOW_NOISE_DRAWS", "FASTVLA_FLOW_STEPS")
K_POL, N_POL, S_POL, A_POL = 8, 3, 4, 14


def _policy(seed=0, **kw):
    from vla_fastvlm.fastvla.configuration_fastvla import FastVLAConfig
    from vla_fastvlm.fastvla.modeling_fastvla import FastVLAPolicy
    torch.manual_seed(seed)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K_POL, n_action_steps=N_POL,
                         action_head="flow", flow_time_dim=6, flow_seed=77, flow_steps=3, **kw).to(DEV)


def _obs():
    g = torch.Generator().manual_seed(5)
    return torch.rand(3, 72, 96, generator=g).to(DEV), torch.randn(14, generator=g).to(DEV), "open drawer"


def _medoid_choice(cands):
    """(B, S, K, A) -> (B,): torch's float64 argmin of the summed squared distances"""
    c = cands.double().flatten(2)
    return (c[:, :, None] - c[:, None]).pow(2).sum(-1).sum(-1).argmin(dim=1)


def _coherent_choice(cands, kept, shift, decay=0.5):
    """(B, S, K, A), (B, K, A) -> (B,): torch's float64 argmin of the weighted squared distance to the kept chunk read `shift` steps ahead"""
    K = cands.shape[2]
    w = torch.tensor([decay ** k for k in range(K - shift)], dtype=torch.float64, device=cands.device)
    d = (cands.double()[:, :, :K - shift] - kept.double()[:, None, shift:]).pow(2).sum(-1)
    return (d * w).sum(-1).argmin(dim=1)


def _close(pol):
    pol.model.backbone.engine().close()


def test_policy_first_serves_a_policy_without_samples_and_off_means_off(monkeypatch, tmp_path):
    import json
    from vla_fastvlm.utils.checkpoint import save_policy_checkpoint
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    img, st, task = _obs()
    plain, first = _policy(), _policy(flow_samples=S_POL, flow_select="first")
    for _ in range(2 * N_POL + 1):                                        # two re-plans: the queue serves the chosen chunk
        assert torch.equal(first.select_action(img, st, task, DEV), plain.select_action(img, st, task, DEV))
    assert torch.equal(first.select_action_chunk(img, st, task, DEV), plain.select_action_chunk(img, st, task, DEV))
    assert first.last_candidates.shape == (1, S_POL, K_POL, A_POL) and first.last_candidates.is_cuda and int(first.last_choice[0]) == 0
    assert first.last_sample_spread.shape == (1, K_POL, A_POL) and float(first.last_sample_spread.min()) > 0
    # off means off: nothing configured, nothing kept, the workspace plan as it was
    assert plain.last_candidates is None and plain.last_choice is None and plain.model._engine().head_flow_samples is None
    assert plain.model._engine().workspace_bytes(1, 16, False) < first.model._engine().workspace_bytes(1, 16, False)
    # a property of the run: the checkpoint gains no key
    a = json.loads((save_policy_checkpoint(plain, tmp_path / "plain") / "hip_extras.json").read_text())
    b = json.loads((save_policy_checkpoint(first, tmp_path / "first") / "hip_extras.json").read_text())
    assert a == b
    _close(plain), _close(first)


def test_policy_medoid_and_num_samples(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    img, st, task = _obs()
    pol = _policy(flow_samples=S_POL)
    assert pol.flow_select == "medoid"
    chunk = pol.select_action_chunk(img, st, task, DEV)
    c = pol.last_candidates
    assert torch.equal(pol.last_choice.long(), _medoid_choice(c)) and torch.equal(chunk, c[0, int(pol.last_choice[0])])
    assert torch.allclose(pol.last_sample_spread, c.std(dim=1, unbiased=False), rtol=1e-4, atol=1e-6)
    with torch.no_grad():
        acts = pol.forward(img.unsqueeze(0), st.unsqueeze(0), [task])
    assert acts.shape == (1, K_POL, A_POL) and torch.equal(pol.last_choice.long(), _medoid_choice(pol.last_candidates))
    two = pol.select_action_chunk(img, st, task, DEV, num_samples=2)
    assert pol.last_candidates.shape == (1, 2, K_POL, A_POL) and torch.equal(two, pol.last_candidates[0, 0]) and pol.model.flow_samples_now == S_POL
    with pytest.raises(ValueError, match="num_samples"):
        pol.select_action_chunk(img, st, task, DEV, num_samples=S_POL + 1)
    _close(pol)


def test_policy_coherent_scores_the_replan_against_the_kept_chunk(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    img, st, task = _obs()
    pol = _policy(flow_samples=S_POL, flow_select="coherent")
    served = [pol.select_action(img, st, task, DEV) for _ in range(N_POL)]               # the first plan: nothing to continue, the medoid
    assert torch.equal(pol.last_choice.long(), _medoid_choice(pol.last_candidates))
    kept = pol.last_candidates[:, int(pol.last_choice[0])].clone()
    assert torch.equal(torch.stack(served), kept[0, :N_POL])
    nxt = pol.select_action(img, st, task, DEV)                                          # the re-plan, read shift = 3 steps ahead
    want = _coherent_choice(pol.last_candidates, kept, N_POL)
    assert torch.equal(pol.last_choice.long(), want) and torch.equal(nxt, pol.last_candidates[0, int(want[0]), 0])
    pol.reset()                                                                          # forgets the kept chunk: the medoid again
    pol.select_action(img, st, task, DEV)
    assert torch.equal(pol.last_choice.long(), _medoid_choice(pol.last_candidates))
    _close(pol)
    # with rtc_method="prefix" the pinned steps of EVERY candidate are the old plan's bits
    D = 2
    pol = _policy(flow_samples=S_POL, flow_select="coherent", rtc=True, rtc_method="prefix", flow_prefix_max_delay=D)
    for _ in range(N_POL):
        pol.select_action(img, st, task, DEV)
    kept = pol.last_chunk_normalised.clone()
    pol.select_action(img, st, task, DEV)
    c = pol.last_candidates
    assert torch.equal(c[0, :, :D], kept[N_POL:N_POL + D].expand(S_POL, D, A_POL))
    assert torch.equal(pol.last_choice.long(), _coherent_choice(c, kept.unsqueeze(0), N_POL))
    assert not torch.equal(c[0, 0, D:], c[0, 1, D:])
    _close(pol)


def test_lerobot_plugin_samples_candidates_for_every_environment(monkeypatch):
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
    pol, plain = make(flow_samples=4), make()
    two = pol.predict_action_chunk(batch, num_samples=2)
    assert pol.last_candidates.shape == (B, 2, K, A) and bool((pol.last_choice == 0).all())      # two candidates tie exactly: the lower index
    assert torch.equal(two, plain.predict_action_chunk(batch)) and torch.equal(two, pol.last_candidates[:, 0])
    four = pol.predict_action_chunk(batch)
    ch = pol.last_choice.long()
    assert torch.equal(ch, _medoid_choice(pol.last_candidates)) and torch.equal(four, pol.last_candidates[torch.arange(B), ch])
    acts = [pol.select_action(batch) for _ in range(3)]                                          # the queue serves the chosen chunks of all B environments
    assert all(a.shape == (B, A) for a in acts)
    with pytest.raises(ValueError, match="num_samples"):
        pol.predict_action_chunk(batch, num_samples=5)
    _close(pol), _close(plain)
