"""Shared by tests/test_augment_host.py and tests/test_gpu_augment.py: an independent numpy statement of the image augmentation's contract
(include/fastvla_hip.h fv_augment_sample / fv_augment_draw / fv_preprocess_augmented).  Nothing here calls the library.

  philox4x32_10   the generator, pinned by the Random123 known answers in the host test
  draw_ref        the table fv_augment_draw must produce, in float64
  augment_ref     the pixels fv_preprocess_augmented must produce from a table, evaluated in a chosen precision: float32 restates the kernel's
                  own arithmetic (every product and sum rounded on its own), float64 is the reference the GPU test bounds the kernel against
"""
from __future__ import annotations

import numpy as np

GRAY = (0.299, 0.587, 0.114)
SAMPLE_FLOATS = 20      # an 80-byte row as 20 fp32 words; word 16 holds the int32 `colour`
SHAPES = {              # name -> (B, C, H, W, dtype, resize_with_padding): the source shapes both test files use
    "f32_30x40": (2, 3, 30, 40, "f32", True),
    "u8_gray_21x21": (1, 1, 21, 21, "u8", True),
    "f32_100x140_down": (2, 3, 100, 140, "f32", True),
    "u8_30x40_stretch": (2, 3, 30, 40, "u8", False),
    "f32_rgba_17x9": (2, 4, 17, 9, "f32", True),
}


def source(name: str, seed: int = 3) -> np.ndarray:
    B, C, H, W, dt, _ = SHAPES[name]
    rng = np.random.default_rng(seed)
    if dt == "u8":
        return rng.integers(0, 256, size=(B, C, H, W), dtype=np.uint8)
    return rng.random((B, C, H, W), dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------ Philox4x32-10
def philox4x32_10(counter, key):
    """counter: 4 arrays of uint32 (broadcastable), key: 2 uint32 -> 4 arrays of uint32 (Salmon et al., Random123)"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def uniforms(B: int, seed: int, offset: int, sample_base: int = 0) -> np.ndarray:
    """(B, 8) float64: u_k = (r_k >> 8) 2^-24 of the two blocks of each sample; counter = (ctr lo, ctr hi, offset lo, offset hi), ctr = 2 (base + b) + {0, 1}"""
    g = np.arange(B, dtype=np.uint64) + np.uint64(sample_base)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.zeros((B, 8))
    for j in (0, 1):
        ctr = np.uint64(2) * g + np.uint64(j)
        r = philox4x32_10((ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), np.full(B, offset & 0xFFFFFFFF, dtype=np.uint64),
                           np.full(B, (offset >> 32) & 0xFFFFFFFF, dtype=np.uint64)), key)
        for k in range(4):
            out[:, 4 * j + k] = (r[k] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return out


# ------------------------------------------------------------------------------------------------------------------ the table
def gray_mean(img: np.ndarray) -> np.ndarray:
    """(B,) float64: the gray mean of each whole source image (one channel: its mean)"""
    x = img.astype(np.float64)
    m = x.reshape(x.shape[0], x.shape[1], -1).mean(axis=2)
    return m[:, 0] if x.shape[1] < 3 else m[:, 0] * GRAY[0] + m[:, 1] * GRAY[1] + m[:, 2] * GRAY[2]


def colour_matrix(b, c, s, mu):
    """M = b c (s I + (1 - s) 1 w^T), o = (1 - c) b mu 1; scalars or (B,) arrays -> (..., 9), (..., 3)"""
    b, c, s, mu = (np.asarray(v, dtype=np.float64) for v in (b, c, s, mu))
    w = np.asarray(GRAY)
    m = (b * c)[..., None, None] * (s[..., None, None] * np.eye(3) + (1.0 - s)[..., None, None] * w[None, :])
    o = ((1.0 - c) * b * mu)[..., None] * np.ones(3)
    return m.reshape(m.shape[:-2] + (9,)), o


def draw_ref(options: dict, B: int, H: int, W: int, seed: int, offset: int, sample_base: int = 0, mu=None) -> dict:
    """float64 statement of fv_augment_draw; options = five (lo, hi) pairs as the fp32 values the library receives.  mu: (B,) gray means (needed when
    contrast is not (1, 1))."""
    f = {k: (float(np.float32(v[0])), float(np.float32(v[1]))) for k, v in options.items()}
    u = uniforms(B, seed, offset, sample_base)
    lerp = lambda r, t: r[0] + (r[1] - r[0]) * t   # noqa: E731
    a = lerp(f["crop_area"], u[:, 0])
    rho = np.exp(lerp((np.log(f["crop_ratio"][0]), np.log(f["crop_ratio"][1])), u[:, 1]))
    cw = np.maximum(np.minimum(W * np.sqrt(a * rho), W), 1.0)
    ch = np.maximum(np.minimum(H * np.sqrt(a / rho), H), 1.0)
    one = lambda k: f[k] == (1.0, 1.0)   # noqa: E731
    colour = not (one("brightness") and one("contrast") and one("saturation"))
    bf, cf, sf = lerp(f["brightness"], u[:, 4]), lerp(f["contrast"], u[:, 5]), lerp(f["saturation"], u[:, 6])
    if colour:
        m, o = colour_matrix(bf, cf, sf, np.zeros(B) if mu is None else mu)
    else:
        m, o = np.tile(np.eye(3).reshape(9), (B, 1)), np.zeros((B, 3))
    return {"x0": u[:, 2] * (W - cw), "y0": u[:, 3] * (H - ch), "cw": cw, "ch": ch, "m": m, "o": o, "colour": int(colour),
            "a": a, "rho": rho, "b": bf, "c": cf, "s": sf, "u": u}


def make_table(x0, y0, cw, ch, m=None, o=None, colour=0) -> np.ndarray:
    """(B, 20) float32 rows from per-sample fields (m, o: (B, 9), (B, 3); default the identity map)"""
    x0 = np.atleast_1d(np.asarray(x0, dtype=np.float32))
    B = x0.shape[0]
    t = np.zeros((B, SAMPLE_FLOATS), dtype=np.float32)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = x0, y0, cw, ch
    t[:, 4:13] = np.eye(3, dtype=np.float32).reshape(9) if m is None else np.asarray(m, dtype=np.float32)
    t[:, 13:16] = 0.0 if o is None else np.asarray(o, dtype=np.float32)
    t.view(np.int32)[:, 16] = colour
    return t


def identity_table(B: int, H: int, W: int) -> np.ndarray:
    return make_table(np.zeros(B), np.zeros(B), np.full(B, W), np.full(B, H))


# ------------------------------------------------------------------------------------------------------------------ the pixels
def letterbox_geometry(H: int, W: int, S: int, resize_with_padding: bool = True):
    if not resize_with_padding:
        return S, S, 0, 0
    ratio = max(W / S, H / S)
    rh, rw = int(H / ratio), int(W / ratio)
    return rh, rw, S - rh, S - rw


def _taps(n_out: int, n_in: int, extent, origin, dt):
    """source taps of one axis: t = (d + 0.5) (extent / n_out) - 0.5, s = max(t + origin, 0), i0 = clamp((int)s), i1 = min(i0 + 1, n_in - 1), w = s - i0;
    every operation rounded in dt; a non-finite s samples index 0"""
    d = np.arange(n_out).astype(dt)
    scale = dt(extent) / dt(n_out)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (d + dt(0.5)) * scale - dt(0.5)
        s = t + dt(origin)
        s = np.where(np.isnan(s), dt(0.0), np.maximum(s, dt(0.0)))
        s = np.where(np.isfinite(s), s, dt(0.0)).astype(dt)
    i0 = np.clip(np.minimum(s, dt(1.0e9)).astype(np.int64), 0, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (s - i0.astype(dt)).astype(dt)


def augment_ref(img: np.ndarray, S: int, pad: float, table: np.ndarray, value_max: float, dtype=np.float64, resize_with_padding: bool = True) -> np.ndarray:
    """(B,C,H,W) u8 | f32 source + (B, 20) fp32 table -> (B,3,S,S) in `dtype` (no bf16 rounding): the contract of fv_preprocess_augmented"""
    dt = np.dtype(dtype).type
    B, C, H, W = img.shape
    rh, rw, pt, pl = letterbox_geometry(H, W, S, resize_with_padding)
    x = img[:, :3] if C >= 3 else img
    x = x.astype(dt)
    out = np.full((B, 3, S, S), dt(np.float32(pad)), dtype=dt)
    colour = np.ascontiguousarray(table).view(np.int32)[:, 16]
    one = dt(1.0)
    for b in range(B):
        x0, y0, cw, ch = (table[b, k] for k in range(4))       # fp32 values, as the kernel reads them
        ix0, ix1, wx = _taps(rw, W, cw, x0, dt)
        iy0, iy1, wy = _taps(rh, H, ch, y0, dt)
        src = x[b]
        wx_, wy_ = wx[None, None, :], wy[None, :, None]
        top, bot = src[:, iy0, :], src[:, iy1, :]
        t0 = (one - wx_) * top[:, :, ix0] + wx_ * top[:, :, ix1]
        t1 = (one - wx_) * bot[:, :, ix0] + wx_ * bot[:, :, ix1]
        v = (one - wy_) * t0 + wy_ * t1
        if v.shape[0] == 1:
            v = np.repeat(v, 3, axis=0)
        if colour[b]:
            m, o = table[b, 4:13].astype(dt).reshape(3, 3), table[b, 13:16].astype(dt)
            v = np.einsum("ij,jyx->iyx", m, v) + o[:, None, None]
            v = np.minimum(np.maximum(v, dt(0.0)), dt(value_max))
        out[b, :, pt:pt + rh, pl:pl + rw] = v
    return out
