"""-m gpu: on-device image augmentation (fv_augment_draw / fv_preprocess_augmented in include/fastvla_hip.h; csrc/augment_kernels.hip;
fastvla_hip/augment.py) against the numpy statement of its contract in tests/augment_util.py.

Bounds, from the arithmetic and not from a run:
  identity   an identity table gives fv_preprocess's output, torch.equal.
  pixels     |got - ref64| <= 2^-8 |ref64| + 1e-4 value_max against the float64 evaluation of the same formulas on the same fp32 table.  The first term is
             bf16's half step at worst; the second is 5x the noise of an fp32 evaluation of these formulas against a float64 one (2.1e-5 value_max, measured
             on the CPU between the two evaluations of tests/augment_util.py, sources up to 336^2).
  table      1e-5 relative for every drawn field against numpy Philox + float64 formulas; the gray mean 1e-6 relative.
  moments    the mean of 4096 draws of a uniform quantity within 5 (hi - lo) / sqrt(12 x 4096) of its centre (five standard errors; the seed is fixed).
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_util as au  # noqa: E402
from gpu_util import DEV  # noqa: E402
from fastvla_hip import FastVLAEngine, FastVLAHipError, arch, augment  # noqa: E402

S, PAD = 64, 0.25


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    m = arch.ModelConfig("lb", arch.LLMConfig(hidden=64, layers=1, heads=2, kv_heads=1, head_dim=32, inter=64, vocab=64),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=S))
    e = FastVLAEngine(m, hidden_dim=32, fusion_dim=32)
    yield e
    e.close()


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _vmax(img: np.ndarray) -> float:
    return 255.0 if img.dtype == np.uint8 else 1.0


def _nchw(pix: torch.Tensor) -> np.ndarray:
    assert float(pix[..., 3].float().abs().max()) == 0.0
    return pix[..., :3].permute(0, 3, 1, 2).float().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("name", list(au.SHAPES))
def test_identity_table_equals_preprocess_bit_for_bit(eng, name):
    B, Cc, H, W, _, rwp = au.SHAPES[name]
    img = _dev(au.source(name))
    want = eng.preprocess(img, pad_value=PAD, resize_with_padding=rwp)
    got = eng.preprocess_augmented(img, _dev(au.identity_table(B, H, W)), pad_value=PAD, resize_with_padding=rwp)
    drawn = eng.augment_draw(augment.normalize_options(), img, seed=5, offset=9)      # every range (1, 1): the rows ARE the identity
    again = eng.preprocess_augmented(img, drawn, pad_value=PAD, resize_with_padding=rwp)
    torch.cuda.synchronize()
    assert np.array_equal(drawn.cpu().numpy().view(np.uint32), au.identity_table(B, H, W).view(np.uint32))
    assert torch.equal(got, want) and torch.equal(again, want)


# ------------------------------------------------------------------------------------------------------------------ 2. explicit tables
def _tables(name: str, img: np.ndarray):
    """(what, table) for one source: random windows (area 0.3 .. 1, ratio 0.5 .. 2), one flush with each border, one partly outside the image; colour
    factors b, c in 0.5 .. 1.5 and s in 0 .. 2 about the image's own gray mean"""
    B, Cc, H, W = img.shape
    rng = np.random.default_rng(sum(map(ord, name)))
    mu = au.gray_mean(img)

    def colour():
        return au.colour_matrix(rng.uniform(0.5, 1.5, B), rng.uniform(0.5, 1.5, B), rng.uniform(0.0, 2.0, B), mu)

    def window():
        a, rho = rng.uniform(0.3, 1.0, B), np.exp(rng.uniform(np.log(0.5), np.log(2.0), B))
        cw, ch = np.clip(W * np.sqrt(a * rho), 1.0, W), np.clip(H * np.sqrt(a / rho), 1.0, H)
        return rng.uniform(0, 1, B) * (W - cw), rng.uniform(0, 1, B) * (H - ch), cw, ch

    out = []
    for i in range(3):
        m, o = colour()
        out.append((f"random window {i}", au.make_table(*window(), m, o, colour=1)))
    out.append(("random window, colour skipped", au.make_table(*window())))
    cw, ch = np.full(B, 0.6 * W), np.full(B, 0.7 * H)
    for what, x0, y0 in (("flush left", 0.0, 0.2 * H), ("flush top", 0.3 * W, 0.0), ("flush right", W - 0.6 * W, 0.1 * H), ("flush bottom", 0.1 * W, H - 0.7 * H)):
        m, o = colour()
        out.append((what, au.make_table(np.full(B, x0), np.full(B, y0), cw, ch, m, o, colour=1)))
    m, o = colour()
    out.append(("partly outside", au.make_table(np.full(B, -0.2 * W), np.full(B, 0.6 * H), np.full(B, 0.8 * W), np.full(B, 0.9 * H), m, o, colour=1)))
    # the extremes of the colour ranges, so that both ends of the clamp are reached whatever the draws above were
    m, o = au.colour_matrix(np.full(B, 1.5), np.full(B, 1.5), np.full(B, 2.0), mu)
    out.append(("full image, strongest colour", au.make_table(np.zeros(B), np.zeros(B), np.full(B, W), np.full(B, H), m, o, colour=1)))
    return out


@pytest.mark.parametrize("name", list(au.SHAPES))
def test_explicit_tables_against_the_float64_restatement(eng, name):
    B, Cc, H, W, _, rwp = au.SHAPES[name]
    img = au.source(name)
    vmax = _vmax(img)
    dimg = _dev(img)
    low = high = 0
    worst = []
    for what, table in _tables(name, img):
        got = _nchw(eng.preprocess_augmented(dimg, _dev(table), pad_value=PAD, resize_with_padding=rwp))
        ref = au.augment_ref(img, S, PAD, table, vmax, dtype=np.float64, resize_with_padding=rwp)
        assert np.isfinite(got).all() and np.isfinite(ref).all()
        rh, rw, pt, pl = au.letterbox_geometry(H, W, S, rwp)
        if table.view(np.int32)[0, 16]:
            region = ref[:, :, pt:, pl:]
            low, high = low + int((region == 0.0).sum()), high + int((region == vmax).sum())
        if pt:
            assert np.array_equal(got[:, :, :pt, :], np.full_like(got[:, :, :pt, :], PAD))      # pad pixels keep pad_value (0.25 is a bf16 number)
        if pl:
            assert np.array_equal(got[:, :, :, :pl], np.full_like(got[:, :, :, :pl], PAD))
        ratio = float((np.abs(got - ref) / (2.0 ** -8 * np.abs(ref) + 1e-4 * vmax)).max())
        worst.append((what, ratio))
        print(f"{name}: {what}: max |got - ref| / bound = {ratio:.3f}")
    assert low > 0 and high > 0, "the tables of this test must reach both ends of the clamp"
    assert all(r <= 1.0 for _, r in worst), worst


# ------------------------------------------------------------------------------------------------------------------ 3. drawing
DRAW = dict(crop_area=(0.3, 0.6), crop_ratio=(0.75, 4.0 / 3.0), brightness=(0.8, 1.2), contrast=(0.5, 1.5), saturation=(0.0, 2.0))


def _fields(table: torch.Tensor) -> dict:
    t = table.cpu().numpy()
    return {"x0": t[:, 0], "y0": t[:, 1], "cw": t[:, 2], "ch": t[:, 3], "m": t[:, 4:13], "o": t[:, 13:16], "colour": np.ascontiguousarray(t).view(np.int32)[:, 16],
            "pad": np.ascontiguousarray(t).view(np.int32)[:, 17:20]}


def test_drawn_table_against_numpy_philox_and_float64_formulas(eng):
    B, H, W = 64, 30, 40
    img = np.random.default_rng(12).random((B, 3, H, W), dtype=np.float32)
    opts = augment.normalize_options(**DRAW)
    seed, offset = (3 << 32) | 77, (1 << 32) + 4
    t = eng.augment_draw(opts, _dev(img), seed=seed, offset=offset)
    t2 = eng.augment_draw(opts, _dev(img), seed=seed, offset=offset)
    other_offset = eng.augment_draw(opts, _dev(img), seed=seed, offset=offset + 1)
    other_seed = eng.augment_draw(opts, _dev(img), seed=seed + 1, offset=offset)
    row7 = eng.augment_draw(opts, _dev(img[7:8]), seed=seed, offset=offset, sample_base=7)
    torch.cuda.synchronize()
    got, ref = _fields(t), au.draw_ref(opts, B, H, W, seed, offset, mu=au.gray_mean(img))
    for k in ("x0", "y0", "cw", "ch", "m", "o"):
        err = float((np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-30)).max())
        print(f"drawn {k}: max relative error {err:.2e}")
        assert err <= 1e-5, k
    assert (got["colour"] == 1).all() and not got["pad"].any()
    # every window inside the image (fp32 rounding of the two fields aside), area and ratio inside the asked ranges
    tol = 1e-5
    assert (got["x0"] >= 0).all() and (got["y0"] >= 0).all() and (got["cw"] >= 1).all() and (got["ch"] >= 1).all()
    assert (got["x0"].astype(np.float64) + got["cw"] <= W * (1 + tol)).all() and (got["y0"].astype(np.float64) + got["ch"] <= H * (1 + tol)).all()
    area = got["cw"].astype(np.float64) * got["ch"] / (H * W)
    rho = (got["cw"].astype(np.float64) / W) / (got["ch"].astype(np.float64) / H)
    assert (area >= 0.3 * (1 - tol)).all() and (area <= 0.6 * (1 + tol)).all() and (rho >= 0.75 * (1 - tol)).all() and (rho <= 4.0 / 3.0 * (1 + tol)).all()
    # reproducible from (seed, offset); the stream belongs to the global sample index
    assert torch.equal(t, t2)
    assert not torch.equal(t, other_offset) and not torch.equal(t, other_seed)
    assert len({tuple(r) for r in t.cpu().numpy()[:, :4].tolist()}) == B            # another sample, another window
    assert torch.equal(row7[0], t[7])


@pytest.mark.parametrize("kind", ["f32", "u8", "u8_gray"])
def test_gray_mean_is_accurate_and_repeatable(eng, kind):
    """brightness (1, 1), contrast (0, 0): c = 0 exactly, so the row's offset IS the gray mean"""
    rng = np.random.default_rng(21)
    B, H, W = 64, 30, 40
    img = rng.random((B, 3, H, W), dtype=np.float32) if kind == "f32" else rng.integers(0, 256, size=(B, 1 if kind == "u8_gray" else 3, H, W), dtype=np.uint8)
    opts = augment.normalize_options(contrast=(0.0, 0.0))
    a, b = eng.augment_draw(opts, _dev(img), seed=1), eng.augment_draw(opts, _dev(img), seed=1)
    torch.cuda.synchronize()
    o = _fields(a)["o"]
    mu = au.gray_mean(img)
    err = float((np.abs(o - mu[:, None]) / mu[:, None]).max())
    print(f"gray mean {kind}: max relative error {err:.2e}")
    assert err <= 1e-6 and torch.equal(a, b)
    assert not _fields(a)["m"].any()        # c = 0: the matrix vanishes, the image collapses onto its mean


# ------------------------------------------------------------------------------------------------------------------ 4. moments
def test_moments_of_4096_draws_without_images(eng):
    B, H, W = 4096, 30, 40
    opts = augment.normalize_options(crop_area=(0.3, 0.6), crop_ratio=(0.75, 4.0 / 3.0), brightness=(0.5, 1.5), saturation=(0.0, 2.0))     # contrast off: img may be null
    f = _fields(eng.augment_draw(opts, None, shape=(B, 3, H, W), seed=2024, offset=3))
    cw, ch, m = f["cw"].astype(np.float64), f["ch"].astype(np.float64), f["m"].astype(np.float64)
    b = m[:, 0:3].sum(axis=1)                                      # a row of b (s I + (1 - s) 1 w^T) sums to b
    s = (m[:, 0] / b - au.GRAY[0]) / (1.0 - au.GRAY[0])
    for what, x, lo, hi in (("a", cw * ch / (H * W), 0.3, 0.6), ("ln rho", np.log((cw / W) / (ch / H)), np.log(0.75), np.log(4.0 / 3.0)), ("b", b, 0.5, 1.5),
                            ("s", s, 0.0, 2.0), ("x0 / (Win - cw)", f["x0"] / (W - cw), 0.0, 1.0)):
        dev, bound = abs(float(x.mean()) - 0.5 * (lo + hi)), 5.0 * (hi - lo) / np.sqrt(12.0 * B)
        print(f"{what}: |mean - centre| = {dev:.2e}, bound {bound:.2e}")
        assert dev <= bound, what
    assert not f["o"].any() and (f["colour"] == 1).all()


def test_argument_errors_are_answered_before_anything_is_enqueued(eng):
    img = _dev(au.source("f32_30x40"))
    ok = augment.normalize_options(**DRAW)

    def bad_draw(**kw):
        with pytest.raises(FastVLAHipError) as ei:
            eng.augment_draw({**ok, **kw.pop("opts", {})}, kw.pop("images", img), **kw)
        assert ei.value.status == -1, str(ei.value)

    bad_draw(opts={"brightness": (1.2, 0.8)})
    bad_draw(opts={"crop_area": (0.0, 0.5)})
    bad_draw(opts={"crop_ratio": (-1.0, 1.0)})
    bad_draw(opts={"saturation": (-0.5, 1.0)})
    bad_draw(opts={"contrast": (float("nan"), 1.0)})
    bad_draw(images=None, shape=(2, 3, 30, 40))                     # contrast is on: the means need the pixels
    bad_draw(images=None, shape=(2, 2, 30, 40), opts={"contrast": (1.0, 1.0)})
    bad_draw(images=None, shape=(0, 3, 30, 40), opts={"contrast": (1.0, 1.0)})
    table = _dev(au.identity_table(2, 30, 40))
    for vm in (0.0, -1.0, float("nan")):
        with pytest.raises(FastVLAHipError) as ei:
            eng.preprocess_augmented(img, table, value_max=vm)
        assert ei.value.status == -1
    pix = torch.empty(2, S, S, 4, dtype=torch.bfloat16, device=DEV)
    lib, st = eng.lib, torch.cuda.current_stream().cuda_stream
    assert lib.fv_preprocess_augmented(eng.h, img.data_ptr(), 0, 2, 3, 30, 40, 0.0, 1, None, 1.0, pix.data_ptr(), st) == -1
    assert lib.fv_preprocess_augmented(eng.h, None, 0, 2, 3, 30, 40, 0.0, 1, table.data_ptr(), 1.0, pix.data_ptr(), st) == -1
    assert lib.fv_augment_draw(eng.h, None, img.data_ptr(), 0, 2, 3, 30, 40, 0, 0, 0, table.data_ptr(), st) == -1
    cfg = augment.config_struct(ok)
    assert lib.fv_augment_draw(eng.h, C.byref(cfg), img.data_ptr(), 0, 2, 3, 30, 40, 0, 0, 0, None, st) == -1
    with pytest.raises(ValueError):
        eng.preprocess_augmented(img, table[:1])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 5. policy level
AUG = dict(crop_area=(0.6, 0.9), crop_ratio=(0.8, 1.25), brightness=(0.7, 1.3), contrast=(0.7, 1.3), saturation=(0.5, 1.5))
LORA = dict(lora_rank=4, lora_alpha=8.0, lora_targets=["q_proj", "v_proj", "down_proj"])


def _fresh(lora=True, aug=None, seed=3):
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    torch.manual_seed(7)
    cfg = FastVLAConfig(vlm_model_name="synthetic:small:43", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)
    p = FastVLAPolicy(cfg).to(DEV)
    if lora:
        p.enable_backbone_training(**LORA)
    if aug is not None:
        p.enable_image_augmentation(**aug, seed=seed)
    return p


def _batches(n, B=2, seed=8, device=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        b = {"images": torch.rand(B, 3, 96, 128, generator=g), "states": torch.randn(B, 14, generator=g), "actions": torch.randn(B, 14, generator=g),
             "tasks": ["pick up the red cube", "open the drawer", "push"][:B]}
        out.append({k: (v.to(device) if device is not None and torch.is_tensor(v) else v) for k, v in b.items()})
    return out


def _close(*pols):
    for p in pols:
        p.model.backbone.engine().close()


def test_eval_paths_never_augment_and_a_training_step_does(monkeypatch):
    monkeypatch.delenv("FASTVLA_IMAGE_AUG", raising=False)
    batch = _batches(1, device=DEV)[0]
    plain, on, degenerate = _fresh(), _fresh(aug=AUG), _fresh(aug={k: (1.0, 1.0) for k in augment.OPTION_KEYS})
    assert plain.model.backbone._augment is None and on.model.backbone._augment["options"] == augment.normalize_options(**AUG)
    acts, losses = [], []
    for p in (plain, on, degenerate):
        p.eval()
        acts.append(p.select_action(batch["images"][0], batch["states"][0], batch["tasks"][0], DEV).clone())
        with torch.no_grad():
            losses.append(p.compute_loss(batch)["loss"].detach().clone())
    torch.cuda.synchronize()
    assert torch.equal(acts[0], acts[1]) and torch.equal(acts[0], acts[2]) and torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2])
    assert on.model.backbone._augment["drawn"] == 0                  # nothing was drawn by the eval-mode calls
    step = []
    for p in (plain, on, degenerate):
        p.train()
        step.append(p.fused_train_step(batch, lr=1e-3)["loss"].detach().clone())
    torch.cuda.synchronize()
    assert on.model.backbone._augment["drawn"] == 1 and on.model.backbone._augment["stepped"] == 1
    assert torch.isfinite(step[1]) and not torch.equal(step[0], step[1])                       # the augmented frames reach the loss ...
    assert torch.equal(step[0], step[2])                                                        # ... and identity rows give the un-augmented run's bits
    for a, b in ((plain._unfrozen.lflat, degenerate._unfrozen.lflat), (plain._unfrozen.m, degenerate._unfrozen.m), (plain._unfrozen.v, degenerate._unfrozen.v)):
        assert torch.equal(a, b)
    assert not torch.equal(plain._unfrozen.lflat, on._unfrozen.lflat)
    # an eval-mode step-side call after training is still un-augmented; PreparedPixels pass through untouched
    on.eval()
    pix = on.processor.prepare_images(batch["images"], DEV)
    assert torch.equal(pix, plain.processor.prepare_images(batch["images"], DEV))
    assert on.model.backbone._prepare_images_tensor(pix, DEV, augment=True) is pix and on.model.backbone._augment["drawn"] == 1
    on.disable_image_augmentation()
    assert on.model.backbone._augment is None
    _close(plain, on, degenerate)


def test_head_only_path_augments_in_splice_mode_and_refuses_normalize_imagenet(monkeypatch):
    monkeypatch.delenv("FASTVLA_IMAGE_AUG", raising=False)
    batch = _batches(1, device=DEV)[0]
    p = _fresh(lora=False)
    p.model.backbone.splice_image_tokens = True
    p.train()
    base = p.prepare_batch(batch)["pooled"].clone()
    p.enable_image_augmentation(**AUG, seed=3)
    first = p.prepare_batch(batch)["pooled"].clone()
    second = p.prepare_batch(batch)["pooled"].clone()            # the next offset: other windows
    p.eval()
    quiet = p.prepare_batch(batch)["pooled"].clone()
    torch.cuda.synchronize()
    assert torch.isfinite(first).all() and not torch.equal(base, first) and not torch.equal(first, second) and torch.equal(base, quiet)
    assert p.model.backbone._augment["drawn"] == 2
    # the prefix cache neither keeps nor serves augmented frames
    p.train()
    p.model.backbone.cache_image_prefix = True
    p.prepare_batch(batch)
    assert not p.model.backbone.__dict__.get("_prefix_cache")
    p.model.backbone.cache_image_prefix = False
    p.model.backbone.config.normalize_imagenet = True
    with pytest.raises(ValueError, match="normalize_imagenet"):
        p.prepare_batch(batch)
    with pytest.raises(ValueError, match="normalize_imagenet"):
        p.enable_image_augmentation()
    p.model.backbone.config.normalize_imagenet = False
    with pytest.raises(ValueError):
        p.enable_image_augmentation(brightness=(1.2, 0.8))
    monkeypatch.setenv("FASTVLA_IMAGE_AUG", "crop_area=0.8:0.9,saturation=0.5:1.5")
    monkeypatch.setenv("FASTVLA_IMAGE_AUG_SEED", "11")
    a = p.enable_image_augmentation()
    assert a["options"] == augment.normalize_options(crop_area=(0.8, 0.9), saturation=(0.5, 1.5)) and a["seed"] == 11
    a = p.enable_image_augmentation(crop_area=0.7, seed=2)           # an explicit argument beats its twin
    assert a["options"] == augment.normalize_options(crop_area=0.7, saturation=(0.5, 1.5)) and a["seed"] == 2
    _close(p)


def test_trainer_runs_are_reproducible_and_resume_bit_for_bit(tmp_path, monkeypatch):
    """Three Trainer steps with augmentation on: two fresh runs agree bit for bit; a run resumed after two steps -- from a save taken while the third batch's
    look-ahead was already prepared, and from one taken with nothing pending -- continues to the three-step run's bits; other options do not resume."""
    from vla_fastvlm.training import Trainer, TrainingConfig
    from vla_fastvlm.utils.checkpoint import read_extras
    monkeypatch.delenv("FASTVLA_IMAGE_AUG", raising=False)
    data = _batches(3)
    tkw = dict(num_epochs=1, learning_rate=1e-3, warmup_ratio=0.5, logging_steps=1000, eval_steps=1000, seed=1)

    def same(x, y):
        return torch.equal(x._unfrozen.lflat, y._unfrozen.lflat) and torch.equal(x._unfrozen.m, y._unfrozen.m) and torch.equal(x._unfrozen.v, y._unfrozen.v)

    a = _fresh(aug=AUG)
    Trainer(a, data, None, TrainingConfig(output_dir=str(tmp_path / "a"), save_steps=2, max_steps=3, **tkw)).fit()       # step-2 is saved with batch 3 prepared
    a2 = _fresh(aug=AUG)
    Trainer(a2, data, None, TrainingConfig(output_dir=str(tmp_path / "a2"), save_steps=1000, max_steps=3, **tkw)).fit()
    plain = _fresh()
    Trainer(plain, data, None, TrainingConfig(output_dir=str(tmp_path / "p"), save_steps=2, max_steps=3, **tkw)).fit()
    torch.cuda.synchronize()
    assert same(a, a2) and not same(a, plain)
    assert a.model.backbone._augment["stepped"] == 3 and a.model.backbone._augment["drawn"] == 3
    ck = tmp_path / "a" / "checkpoints" / "step-2"
    opt = torch.load(ck / "optimizer.pt", map_location="cpu")
    popt = torch.load(tmp_path / "p" / "checkpoints" / "step-2" / "optimizer.pt", map_location="cpu")
    assert "augment" not in popt and sorted(opt) == sorted(list(popt) + ["augment"])           # a plain run's key list is what it was
    assert opt["augment"] == {"options": augment.record(augment.normalize_options(**AUG)), "seed": 3, "batches": 2}
    json.dumps(opt["augment"])
    assert read_extras(ck)["augment"] == {"options": opt["augment"]["options"], "seed": 3}
    assert "augment" not in read_extras(tmp_path / "p" / "checkpoints" / "step-2")

    b = _fresh(aug=AUG)
    tb = Trainer(b, data[:2], None, TrainingConfig(output_dir=str(tmp_path / "b"), save_steps=2, max_steps=3, **tkw))     # the loader ends at the save: nothing pending
    tb.num_training_steps = 3
    tb.fit()
    for what, src, kw in (("look-ahead pending", ck, dict(lora=False)), ("nothing pending", tmp_path / "b" / "checkpoints" / "step-2", dict(aug=AUG))):
        c = _fresh(**kw)                                        # (lora=False, no augmentation: both come back with the run)
        tc = Trainer(c, data[2:], None, TrainingConfig(output_dir=str(tmp_path / "c"), save_steps=1000, max_steps=3, resume_from=str(src), **tkw))
        tc.num_training_steps = 3
        tc.fit()
        torch.cuda.synchronize()
        assert tc.global_step == 3 and c._unfrozen.step_count == 3, what
        assert c.model.backbone._augment["options"] == a.model.backbone._augment["options"] and c.model.backbone._augment["stepped"] == 3, what
        assert same(c, a), what
        _close(c)
    d = _fresh(aug={**AUG, "brightness": (0.9, 1.1)})          # a run that asks for other options does not resume
    td = Trainer(d, data[2:], None, TrainingConfig(output_dir=str(tmp_path / "d"), save_steps=1000, max_steps=3, resume_from=str(ck), **tkw))
    with pytest.raises(ValueError) as ei:
        td.fit()
    assert "[0.7, 1.3]" in str(ei.value) and "[0.9, 1.1]" in str(ei.value)
    bb = d.model.backbone                                       # ... nor one with another seed, nor an augmented run from a plain run's checkpoint
    bb.enable_image_augmentation(**AUG, seed=4)
    with pytest.raises(ValueError, match="seed 4"):
        bb.load_augmentation_record(opt["augment"])
    with pytest.raises(ValueError, match="without image augmentation"):
        bb.load_augmentation_record(popt.get("augment"))
    bb.disable_image_augmentation()
    bb.load_augmentation_record(None)                           # plain onto plain: nothing to do
    assert bb._augment is None
    _close(a, a2, plain, b, d)
