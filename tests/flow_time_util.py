"""Float64 reference of the flow head's training-time distributions (fv_head_set_flow_time; tests only).

The contract, on the Philox integers tests/flow_util.py reproduces: k = r.x >> 8 of the group-0 block of (row, offset + (s << 56)) is the 24-bit integer
behind the uniform t.  u = k 2^-24, or (s + k 2^-24) / S for draw s of S stratified draws (one float64 division).  tau = F^-1(u):
    uniform        tau = u
    beta(a, b)     tau = I^-1_u(a, b)                      scipy.special.betaincinv
    logit-normal   tau = sigmoid(a + b Phi^-1(u))          scipy.special.ndtri; stratified only (u = 0 gives tau = 0) -- without strata the device keeps its
                                                           fp32 Box-Muller form, flow_util.draw_t_logit_normal's
a, b, t_lo and t_hi are THE fp32 VALUES the spec carries (0.3 is not 0.3 there), everything else float64: t = t_lo + (t_hi - t_lo) tau, which the device rounds
to fp32 once.

The bar of the GPU tests: |t - fl32(t_ref)| <= one fp32 ulp at max(t_ref, 2^-24) -- one rounding of a float64 result whose own error is far below fp32
(tests/test_flow_time_host.py holds the reference to closed forms and to its own round trip, more than three orders of magnitude inside that)."""
from __future__ import annotations

import numpy as np
from scipy import special

import flow_util as fu

U24 = 2.0 ** -24
BETAS = ((1.5, 1.0), (1.0, 1.0), (0.5, 0.5), (2.0, 5.0), (8.0, 0.75), (0.25, 4.0))
RANGES = ((0.0, 1.0), (0.001, 1.0))
BATCHES, DRAWS = (1, 9, 67), (1, 3, 16)
EDGE_K = (0, 1, 2, 1000, 2 ** 20, 2 ** 23, 2 ** 24 - 2, 2 ** 24 - 1)


def draw_k(B: int, seed: int, offset: int) -> np.ndarray:
    """(B,) uint32: the 24-bit integer behind row b's uniform, word x of counter (0, row, offset) >> 8"""
    r = fu._philox(np.zeros(B, np.uint64), np.arange(B, dtype=np.uint64), seed, offset)
    return (r[0] >> np.uint32(8)).astype(np.uint32)


def uniform_u(k, s: int = 0, S: int = 1, stratify: bool = False) -> np.ndarray:
    """float64 u of draw s of S: k 2^-24, or (s + k 2^-24) / S when stratified with S > 1"""
    u = np.asarray(k, np.float64) * U24
    return (float(s) + u) / float(S) if stratify and S > 1 else u


def tau_ref(dist: str, a: float, b: float, u) -> np.ndarray:
    """float64 tau = F^-1(u), from THE fp32 VALUES of a and b the spec carries"""
    u = np.asarray(u, np.float64)
    a, b = float(np.float32(a)), float(np.float32(b))
    if dist == "uniform":
        return u.copy()
    if dist == "beta":
        return special.betaincinv(float(a), float(b), u)
    if dist == "logit_normal":
        with np.errstate(over="ignore", divide="ignore"):
            tau = 1.0 / (1.0 + np.exp(-(float(a) + float(b) * special.ndtri(u))))
        return np.where(u <= 0.0, 0.0, tau)
    raise ValueError(dist)


def scale_ref(tau, t_lo: float, t_hi: float) -> np.ndarray:
    """float64 t = t_lo + (t_hi - t_lo) tau from the fp32 values of the range"""
    lo, hi = float(np.float32(t_lo)), float(np.float32(t_hi))
    return lo + (hi - lo) * np.asarray(tau, np.float64)


def draw_t_ref(B: int, S: int, seed: int, offset: int, dist: str, a: float, b: float, t_lo: float = 0.0, t_hi: float = 1.0, stratify: bool = False) -> np.ndarray:
    """(S B,) float64, draw-major: the reference time of head row s B + b (logit-normal without strata: the Box-Muller form in float64)"""
    out = np.empty(S * B)
    for s in range(S):
        o = offset + (s << 56)
        if dist == "logit_normal" and not (stratify and S > 1):
            tau = fu.draw_t_logit_normal(B, seed, o, a, b)
        else:
            tau = tau_ref(dist, a, b, uniform_u(draw_k(B, seed, o), s, S, stratify))
        out[s * B:(s + 1) * B] = scale_ref(tau, t_lo, t_hi)
    return out


def time_bar(t_ref) -> np.ndarray:
    """one fp32 ulp at max(t_ref, 2^-24)"""
    return fu.ulp32(np.maximum(np.asarray(t_ref, np.float64), U24))


def time_error(t_got, t_ref) -> np.ndarray:
    """|t - fl32(t_ref)| / bar, per row"""
    t_ref = np.asarray(t_ref, np.float64)
    return np.abs(np.asarray(t_got, np.float64) - t_ref.astype(np.float32).astype(np.float64)) / time_bar(t_ref)


# ------------------------------------------------------------------------------------------------------------------ loss by time bucket
def bucket_of(t, n_buckets: int) -> np.ndarray:
    """the device's rule on the fp32 t: min(n - 1, int(fl32(clamp(t, 0, 1) * n)))"""
    tc = np.clip(np.asarray(t, np.float32), np.float32(0), np.float32(1))
    return np.minimum(n_buckets - 1, (tc * np.float32(n_buckets)).astype(np.float32).astype(np.int64))


def loss_per_time_ref(v, u, t, n_buckets: int, pad=None, B=None, K: int = 1):
    """float64: (n_buckets,) sums of (v - u)^2 over the non-padded elements and (n_buckets,) counts.  v, u: (R, da); t: (R,); pad: (B, K) bool or None, row r
    reads the mask of observation r % B"""
    v, u = np.asarray(v, np.float64), np.asarray(u, np.float64)
    R, da = v.shape
    keep = np.ones((R, da), bool)
    if pad is not None:
        pad = np.asarray(pad, bool)
        keep = ~np.repeat(pad[np.arange(R) % B], da // K, axis=1)
    bk = bucket_of(t, n_buckets)
    sq = np.where(keep, (v - u) ** 2, 0.0)
    sums = np.array([sq[bk == j].sum() for j in range(n_buckets)])
    counts = np.array([keep[bk == j].sum() for j in range(n_buckets)], np.int64)
    return sums, counts
