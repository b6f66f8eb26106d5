"""-m gpu: temporal ensembling of action chunks on the device (fv_ensemble_*; fastvla_hip/ensemble.py) -- every served action against the float64 closed
form over 3K + 2 steps (the ring wraps three times), the bit rules (K = 1, the first step after a reset, two runs, one environment reset among many, NaN
in one environment), argument checks, and select_action of both policy surfaces.

Bar per served element: 6 K 2^-24 max|chunk| (ensemble_util.error_bar: derived from the operation count, not measured; test_ensemble_host.py holds an fp32
emulation of the online form below a quarter of it)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ensemble_util import ensemble_closed, error_bar  # noqa: E402
from gpu_util import DEV, stream  # noqa: E402
import fastvla_hip  # noqa: E402
from fastvla_hip import FastVLAEngine, TemporalEnsembler, arch  # noqa: E402
from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy  # noqa: E402

SHAPES = [(1, 1, 1), (1, 2, 1), (3, 4, 5), (2, 7, 3), (5, 8, 14), (64, 50, 14)]
COEFFS = [0.01, 0.0, -0.5, 2.0]


@pytest.fixture(scope="module")
def eng():
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=48, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    e = FastVLAEngine(m, state_dim=6, action_dim=5, hidden_dim=24, fusion_dim=40, max_batch=1)      # the ensembler only needs a handle
    yield e
    e.close()


def _chunks(n_env, K, A, seed):
    """(3K + 2, n_env, K, A) f32 of about N(0, 3^2)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3 * K + 2, n_env, K, A, generator=g) * 3.0


def _run(eng, chunks, coeff, resets=None):
    """chunks (T, n_env, K, A) f32 CPU; resets {step: [env or None, ...]} applied BEFORE that step -> (T, n_env, A) f32 CPU.  No synchronisation in the loop."""
    T, n_env, K, A = chunks.shape
    dev = chunks.to(DEV).contiguous()
    out = torch.full((T, n_env, A), float("nan"), device=DEV)
    ens = TemporalEnsembler(eng, n_env, K, A, coeff)
    for t in range(T):
        for e in (resets or {}).get(t, []):
            ens.reset(e)
        ens.step(dev[t], out=out[t])
    torch.cuda.synchronize()
    ens.close()
    return out.cpu()


@pytest.mark.parametrize("coeff", COEFFS)
@pytest.mark.parametrize("shape", SHAPES)
def test_step_matches_the_float64_closed_form(eng, shape, coeff):
    n_env, K, A = shape
    chunks = _chunks(n_env, K, A, seed=K * 100 + A)
    got = _run(eng, chunks, coeff)
    ref = ensemble_closed(chunks.numpy(), coeff)
    bar = error_bar(K, float(chunks.abs().max()))
    err = float((got.double() - torch.from_numpy(ref)).abs().max())
    print(f"[ensemble {shape} coeff={coeff}] worst error / bar {err / bar:.3f} (bar {bar:.3e})")
    assert torch.isfinite(got).all() and err <= bar, (err, bar)
    assert torch.equal(got[0], chunks[0, :, 0])                               # nothing to average yet: the chunk's row, bit for bit
    if K == 1:
        assert torch.equal(got, chunks[:, :, 0])
    assert torch.equal(_run(eng, chunks, coeff), got)                         # two runs agree bit for bit


@pytest.mark.parametrize("shape", [(3, 4, 5), (5, 8, 14)])
def test_resetting_one_environment_leaves_the_others_alone(eng, shape):
    n_env, K, A = shape
    coeff, e, at = 0.01, 1, K + 2
    chunks = _chunks(n_env, K, A, seed=7)
    plain, reset = _run(eng, chunks, coeff), _run(eng, chunks, coeff, {at: [e]})
    others = [i for i in range(n_env) if i != e]
    assert torch.equal(reset[:, others], plain[:, others])                    # bit-identical to the run without the reset
    assert torch.equal(reset[:at, e], plain[:at, e]) and not torch.equal(reset[at:, e], plain[at:, e])
    assert torch.equal(reset[at, e], chunks[at, e, 0])                        # the first step after the reset: the chunk's row, bit for bit
    # ... and from there the reset environment is a fresh history: the bits of a run that starts at that step
    fresh = _run(eng, chunks[at:, e:e + 1].contiguous(), coeff)
    assert torch.equal(reset[at:, e], fresh[:, 0])
    ref = ensemble_closed(chunks.numpy(), coeff, {at: [e]})
    assert float((reset.double() - torch.from_numpy(ref)).abs().max()) <= error_bar(K, float(chunks.abs().max()))
    # reset of all (env = None -> -1)
    every = _run(eng, chunks, coeff, {at: [None]})
    assert torch.equal(every[at], chunks[at, :, 0]) and torch.equal(every[at:, e], reset[at:, e])


def test_nan_in_one_environment_reaches_no_other(eng):
    n_env, K, A = 5, 8, 14
    chunks = _chunks(n_env, K, A, seed=9)
    dirty = chunks.clone()
    dirty[K + 1, 2] = float("nan")                                            # the whole chunk environment 2 predicts at step K + 1
    plain, got = _run(eng, chunks, 0.01), _run(eng, dirty, 0.01)
    others = [0, 1, 3, 4]
    assert torch.equal(got[:, others], plain[:, others])
    assert torch.equal(got[:K + 1, 2], plain[:K + 1, 2])
    assert torch.isnan(got[K + 1:2 * K + 1, 2]).all()                         # the K time steps that chunk speaks about
    assert torch.equal(got[2 * K + 1:, 2], plain[2 * K + 1:, 2])              # their slots are served and start over: the NaN does not linger


def test_bad_arguments_return_err_arg_and_touch_nothing(eng):
    L = fastvla_hip.load()
    out = C.c_void_p()
    for args in ((0, 4, 5, 0.01), (3, 0, 5, 0.01), (3, 4, 0, 0.01), (-1, 4, 5, 0.01), (3, 4, 5, float("nan")), (3, 4, 5, float("inf")), (3, 4, 5, float("-inf"))):
        assert L.fv_ensemble_create(eng.h, *args, C.byref(out)) == -1 and not out.value, args
    assert L.fv_ensemble_create(eng.h, 3, 4, 5, 0.01, None) == -1 and L.fv_ensemble_create(None, 3, 4, 5, 0.01, C.byref(out)) == -1
    for bad in ((0, 4, 5, 0.1), (3, 4, 5, float("nan"))):
        with pytest.raises(ValueError):
            TemporalEnsembler(eng, *bad)
    n_env, K, A = 3, 4, 5
    chunks = _chunks(n_env, K, A, seed=3)
    dev = chunks.to(DEV)
    control = _run(eng, chunks, 0.5)
    ens = TemporalEnsembler(eng, n_env, K, A, 0.5)
    got = torch.full((chunks.shape[0], n_env, A), float("nan"), device=DEV)
    sentinel = torch.full((n_env, A), 7.0, device=DEV)
    for t in range(chunks.shape[0]):
        if t == K + 1:                                                        # mid-run: every refused call leaves the ring, its position and `actions` as they were
            assert L.fv_ensemble_step(eng.h, ens.handle(), None, sentinel.data_ptr(), stream()) == -1
            assert L.fv_ensemble_step(eng.h, ens.handle(), dev[t].data_ptr(), None, stream()) == -1
            assert L.fv_ensemble_step(eng.h, None, dev[t].data_ptr(), sentinel.data_ptr(), stream()) == -1
            assert L.fv_ensemble_step(None, ens.handle(), dev[t].data_ptr(), sentinel.data_ptr(), stream()) == -1
            for env in (-2, n_env, 1 << 20):
                assert L.fv_ensemble_reset(eng.h, ens.handle(), env, stream()) == -1
            assert b"env" in L.fv_last_error(eng.h)
            assert L.fv_ensemble_reset(eng.h, None, 0, stream()) == -1
            with pytest.raises(ValueError):
                ens.reset(n_env)
            with pytest.raises(ValueError):
                ens.step(dev[t][:, :2])
        ens.step(dev[t], out=got[t])
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all()) and torch.equal(got.cpu(), control)
    assert L.fv_ensemble_destroy(eng.h, None) == 0 and L.fv_ensemble_destroy(None, ens.handle()) == -1
    ens.close()
    with pytest.raises(fastvla_hip.FastVLAHipError):
        ens.step(dev[0])


# ------------------------------------------------------------------------------------------------------------------ the policy surfaces
def _core_policy(K, **kw):
    torch.manual_seed(31)
    return FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=K, **kw).to(DEV)


def test_core_select_action_is_the_ensemble_of_its_chunks():
    K, coeff = 4, 0.01
    pol = _core_policy(K, temporal_ensemble_coeff=coeff)
    A, T, dev = pol.config.action_dim, 2 * K + 1, torch.device(DEV)
    g = torch.Generator().manual_seed(9)
    obs = [(torch.rand(3, 72, 96, generator=g), torch.randn(14, generator=g)) for _ in range(T)]
    chunks = torch.stack([pol.select_action_chunk(img, st, "stack the red block", dev).cpu() for img, st in obs])      # (T, K, A)
    assert chunks.shape == (T, K, A)
    pol.reset()
    got = torch.stack([pol.select_action(img, st, "stack the red block", dev) for img, st in obs]).cpu()
    assert got.shape == (T, A) and len(pol._action_queue) == 0
    ref = ensemble_closed(chunks.unsqueeze(1).numpy(), coeff)[:, 0]
    bar = error_bar(K, float(chunks.abs().max()))
    err = float((got.double() - torch.from_numpy(ref)).abs().max())
    print(f"[ensemble core policy K={K}] worst error / bar {err / bar:.3f}")
    assert err <= bar and torch.equal(got[0], chunks[0, 0])
    assert not torch.equal(got[K], chunks[K, 0])                              # it IS an average
    pol.reset()                                                               # restarts: the next action is its chunk's row 0 again
    assert torch.equal(pol.select_action(*obs[3], "stack the red block", dev).cpu(), chunks[3, 0])
    # without the option: today's loop, row 0 of every chunk
    plain = _core_policy(K)
    assert plain.temporal_ensemble_coeff is None
    assert torch.equal(plain.select_action(*obs[1], "stack the red block", dev).cpu(), chunks[1, 0])
    for p_ in (pol, plain):
        p_.model.backbone.engine().close()


def test_lerobot_surface_ensembles_the_batch():
    from vla_fastvlm.lerobot_fastvla import FastVLAConfig as LRConfig, FastVLAPolicy as LRPolicy
    from vla_fastvlm.lerobot_fastvla._lerobot_compat import ACTION, FeatureType, PolicyFeature
    K, A, B, coeff = 4, 5, 3, -0.5
    feats = {"observation.images.top": PolicyFeature(type=FeatureType.VISUAL, shape=(3, 64, 64)), "observation.state": PolicyFeature(type=FeatureType.STATE, shape=(6,))}
    cfg = LRConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=32, fusion_dim=48, input_features=feats, chunk_size=K, n_action_steps=1,
                   output_features={ACTION: PolicyFeature(type=FeatureType.ACTION, shape=(A,))}, dropout=0.0)
    torch.manual_seed(3)
    pol = LRPolicy(cfg, temporal_ensemble_coeff=coeff).to(DEV)
    g = torch.Generator().manual_seed(4)
    stats = {"observation.state": {"mean": torch.randn(6, generator=g), "std": torch.rand(6, generator=g) + 0.5},
             ACTION: {"mean": torch.randn(A, generator=g), "std": torch.rand(A, generator=g) + 0.5}}
    pol.fold_dataset_stats(stats)                                             # the chunks arrive un-normalised; the mean of an affine map is the affine map of the mean
    T = 2 * K + 1
    batches = [{"observation.images.top": torch.rand(B, 3, 64, 64, generator=g).to(DEV), "observation.state": (torch.randn(B, 6, generator=g) * 2 + 1).to(DEV),
                "task": ["a", "b", "c"]} for _ in range(T)]
    chunks = torch.stack([pol.predict_action_chunk(b).cpu() for b in batches])                  # (T, B, K, A)
    pol.reset()
    got = torch.stack([pol.select_action(b) for b in batches]).cpu()
    assert got.shape == (T, B, A)
    ref = ensemble_closed(chunks.numpy(), coeff)
    bar = error_bar(K, float(chunks.abs().max()))
    err = float((got.double() - torch.from_numpy(ref)).abs().max())
    print(f"[ensemble lerobot surface B={B} K={K}] worst error / bar {err / bar:.3f}")
    assert err <= bar and torch.equal(got[0], chunks[0, :, 0])
    two = {k: v[:2] for k, v in batches[0].items()}
    with pytest.raises(ValueError, match="reset"):
        pol.select_action(two)                                                # another B without a reset()
    pol.reset()
    assert torch.equal(pol.select_action(two).cpu(), chunks[0, :2, 0])
    pol.model.backbone.engine().close()
