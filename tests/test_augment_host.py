"""CPU: the host half of the image augmentation (fastvla_hip/augment.py) and the numpy statement of its contract that the GPU tests bound the kernels
against (tests/augment_util.py): options and environment twins, struct sizes, Philox4x32-10 against the Random123 known answers, the identity table
against the oracle's letterbox bit for bit, and the colour matrix against the composed brightness -> contrast -> saturation."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_util as au
from fastvla_hip import augment
from oracle import preprocess


# ------------------------------------------------------------------------------------------------------------------ options / twins / structs
def test_struct_sizes_and_field_offsets():
    assert C.sizeof(augment.AugmentConfig) == 40 and C.sizeof(augment.AugmentSample) == 80
    assert augment.SAMPLE_FLOATS == au.SAMPLE_FLOATS == 20
    s = augment.AugmentSample
    assert (s.x0.offset, s.y0.offset, s.cw.offset, s.ch.offset, s.m.offset, s.o.offset, s.colour.offset, s.pad.offset) == (0, 4, 8, 12, 16, 52, 64, 68)
    cfg = augment.config_struct(augment.normalize_options(crop_area=(0.5, 0.75), contrast=2))
    assert list(cfg.crop_area) == [0.5, 0.75] and list(cfg.contrast) == [2.0, 2.0] and list(cfg.crop_ratio) == [1.0, 1.0]
    assert [f[0] for f in augment.AugmentConfig._fields_] == ["crop_area", "crop_ratio", "brightness", "contrast", "saturation"]


def test_options_normalise_and_reject():
    assert augment.normalize_options() == augment.IDENTITY and augment.is_identity(augment.normalize_options())
    assert augment.is_identity(None) and augment.is_identity({})
    o = augment.normalize_options(crop_area=0.9, crop_ratio=[0.75, 4 / 3], brightness=(0.8, 1.2))
    assert o["crop_area"] == (0.9, 0.9) and o["crop_ratio"] == (0.75, 4 / 3) and o["contrast"] == (1.0, 1.0) and not augment.is_identity(o)
    assert not augment.is_identity(augment.normalize_options(saturation=(1.0, 1.5)))
    p = augment.preset("default")
    assert p == {"crop_area": (0.9, 0.9), "crop_ratio": (1.0, 1.0), "brightness": (0.8, 1.2), "contrast": (0.8, 1.2), "saturation": (0.8, 1.2)}
    assert augment.from_record(augment.record(p)) == p
    for bad in (dict(crop_area=(0.9, 0.5)), dict(brightness=(1.2, 0.8)), dict(crop_area=0.0), dict(crop_area=(-0.1, 0.5)), dict(crop_ratio=(0.0, 1.0)),
                dict(crop_ratio=-1), dict(brightness=(-0.1, 1.0)), dict(contrast=-1), dict(saturation=(-2, -1)), dict(crop_area=(0.5, 1.5)),
                dict(brightness=float("nan")), dict(contrast=(0.5, float("inf"))), dict(saturation="much"), dict(crop_area=(0.1, 0.2, 0.3))):
        with pytest.raises(ValueError):
            augment.normalize_options(**bad)
    with pytest.raises(ValueError):
        augment.preset("nope")


def test_environment_twins():
    assert augment.options_from_env({}) is None and augment.options_from_env({"FASTVLA_IMAGE_AUG": "0"}) is None
    assert augment.options_from_env({"FASTVLA_IMAGE_AUG": " "}) is None
    assert augment.options_from_env({"FASTVLA_IMAGE_AUG": "1"}) == augment.preset("default")
    o = augment.options_from_env({"FASTVLA_IMAGE_AUG": "crop_area=0.9:0.9, brightness=0.8:1.2,saturation=0.5"})
    assert o == augment.normalize_options(crop_area=(0.9, 0.9), brightness=(0.8, 1.2), saturation=0.5)
    for bad in ("crop_area", "crop_area=", "hue=0.1:0.2", "crop_area=0.9:0.9,crop_area=0.8:0.8", "brightness=a:b", "brightness=1.2:0.8", "crop_area=0:1"):
        with pytest.raises(ValueError):
            augment.options_from_env({"FASTVLA_IMAGE_AUG": bad})
    assert augment.seed_from_env({}) == 0 and augment.seed_from_env({"FASTVLA_IMAGE_AUG_SEED": "17"}) == 17
    for bad in ("x", "-1", "1.5"):
        with pytest.raises(ValueError):
            augment.seed_from_env({"FASTVLA_IMAGE_AUG_SEED": bad})
    # resolve(): nothing explicit and no twin -> the preset; the twin fills what the call leaves open; an explicit argument beats its twin
    assert augment.resolve(environ={}) == (augment.preset("default"), 0)
    assert augment.resolve(crop_area=0.8, environ={}) == (augment.normalize_options(crop_area=0.8), 0)
    env = {"FASTVLA_IMAGE_AUG": "crop_area=0.7:0.9,contrast=0.5:1.5", "FASTVLA_IMAGE_AUG_SEED": "5"}
    assert augment.resolve(environ=env) == (augment.normalize_options(crop_area=(0.7, 0.9), contrast=(0.5, 1.5)), 5)
    assert augment.resolve(crop_area=1.0, seed=9, environ=env) == (augment.normalize_options(contrast=(0.5, 1.5)), 9)
    with pytest.raises(ValueError):
        augment.resolve(brightness=(2, 1), environ={})


# ------------------------------------------------------------------------------------------------------------------ the generator
def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    z = au.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(v) for v in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    o = au.philox4x32_10((f, f, f, f), (f, f))
    assert [int(v) for v in o] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # vectorised over the counter, and the uniforms' convention: 24 bits, [0, 1)
    both = au.philox4x32_10((np.array([0, f]), np.array([0, f]), np.array([0, f]), np.array([0, f])), (0, 0))
    assert [int(v[0]) for v in both] == [int(v) for v in z]
    u = au.uniforms(64, seed=(7 << 32) | 3, offset=(1 << 33) + 5, sample_base=(1 << 32) - 2)
    assert u.shape == (64, 8) and float(u.min()) >= 0.0 and float(u.max()) < 1.0 and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    assert np.array_equal(au.uniforms(1, seed=(7 << 32) | 3, offset=(1 << 33) + 5, sample_base=(1 << 32) - 2 + 9)[0], u[9])


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(au.SHAPES))
def test_fp32_restatement_with_the_identity_table_is_the_oracle_letterbox_bitwise(name):
    B, Cc, H, W, _, rwp = au.SHAPES[name]
    S, pad = 64, 0.25
    img = au.source(name)
    got = au.augment_ref(img, S, pad, au.identity_table(B, H, W), 255.0 if img.dtype == np.uint8 else 1.0, dtype=np.float32, resize_with_padding=rwp)
    ref = preprocess.letterbox(torch.from_numpy(img), S, pad_value=pad, resize_with_padding=rwp).numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape == (B, 3, S, S)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_restatement_windows_taps_and_clamps():
    """a window is a view into the real image: shifting it by whole pixels at scale 1 reads the shifted pixels; out-of-image taps replicate the edge; a
    non-finite coordinate samples index 0"""
    rng = np.random.default_rng(0)
    img = rng.random((1, 3, 64, 64), dtype=np.float32)
    S = 32
    t = au.make_table([5.0], [9.0], [32.0], [32.0])       # a 32 x 32 window at (5, 9): scale 1, taps on pixel centres
    got = au.augment_ref(img, S, 0.0, t, 1.0)
    assert np.allclose(got[0], img[0, :, 9:41, 5:37], atol=0, rtol=0)
    t = au.make_table([40.0], [-8.0], [32.0], [32.0])     # partly outside: columns past 63 repeat column 63, rows above 0 repeat row 0
    got = au.augment_ref(img, S, 0.0, t, 1.0)
    assert np.array_equal(got[0][:, 8:, :24], img[0, :, 0:24, 40:64].astype(np.float64))
    assert np.allclose(got[0][:, :8, :24], img[0, :, 0:1, 40:64]) and np.allclose(got[0][:, 8:, 24:], img[0, :, 0:24, 63:64], rtol=1e-6)
    for bad in (np.nan, np.inf, -np.inf):
        got = au.augment_ref(img, S, 0.0, au.make_table([bad], [0.0], [64.0], [64.0]), 1.0, dtype=np.float32)
        assert got.shape == (1, 3, S, S)


def test_colour_matrix_is_brightness_then_contrast_then_saturation():
    """M v + o against the three steps composed one after the other (no intermediate clamp), and (1 - c) b mu against the composed offset, to 1e-6"""
    rng = np.random.default_rng(4)
    w = np.asarray(au.GRAY)
    for _ in range(32):
        b, c, s = rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5), rng.uniform(0.0, 2.0)
        img = rng.random((3, 6, 7))
        mu = float(w @ img.reshape(3, -1).mean(axis=1))
        m, o = au.colour_matrix(b, c, s, mu)
        v = img * b                                                 # brightness
        v = c * v + (1.0 - c) * (b * mu)                            # contrast about the gray mean of the brightened image (= b mu)
        gray = np.einsum("c,cyx->yx", w, v)
        v = s * v + (1.0 - s) * gray[None]                          # saturation
        got = np.einsum("ij,jyx->iyx", m.reshape(3, 3), img) + o[:, None, None]
        assert np.abs(got - v).max() <= 1e-6
        composed_offset = v - np.einsum("ij,jyx->iyx", m.reshape(3, 3), img)
        assert np.abs(composed_offset - (1.0 - c) * b * mu).max() <= 1e-6
    m, o = au.colour_matrix(1.0, 1.0, 1.0, 0.3)
    assert np.array_equal(m, np.eye(3).reshape(9)) and np.array_equal(o, np.zeros(3))


def test_draw_ref_identity_config_and_ranges():
    ident = {k: (1.0, 1.0) for k in augment.OPTION_KEYS}
    d = au.draw_ref(ident, 8, 30, 40, seed=1, offset=2)
    assert d["colour"] == 0 and np.array_equal(d["cw"], np.full(8, 40.0)) and np.array_equal(d["ch"], np.full(8, 30.0))
    assert not d["x0"].any() and not d["y0"].any() and np.array_equal(d["m"], np.tile(np.eye(3).reshape(9), (8, 1))) and not d["o"].any()
    opts = augment.normalize_options(crop_area=(0.3, 0.6), crop_ratio=(0.75, 4 / 3), brightness=(0.8, 1.2))
    d = au.draw_ref(opts, 64, 30, 40, seed=1, offset=2)
    assert d["colour"] == 1 and (d["x0"] >= 0).all() and (d["x0"] + d["cw"] <= 40 + 1e-9).all() and (d["y0"] + d["ch"] <= 30 + 1e-9).all()
    assert np.allclose(d["cw"] * d["ch"] / 1200.0, d["a"]) and np.allclose((d["cw"] / 40) / (d["ch"] / 30), d["rho"])
