"""Several samples per observation, one chosen on the device (fv_head_flow_sample_multi; tests only): the float64 reference of the scores, the choice and the
spread, an fp32 CPU emulation of the selection kernel's sums (used ONLY to calibrate the GPU bar), the selection cases host and GPU tests share, and the
two-mode toy that shows why a chosen candidate, not an averaged one, is the answer.

Candidates are sample-major as on the device: cand[s, b] is candidate s of observation b, shape (S, B, da) here.
    medoid    score[b, s] = sum_s' sum_e (x_s[e] - x_s'[e])^2
    coherent  score[b, s] = sum_{k < K - shift} w[k] sum_a (x_s[k, a] - prev[b, k + shift, a])^2; a weight of 0 drops its step whatever it holds; a row whose
              row_mask is 0 takes the medoid score
    first     the medoid scores, candidate 0 chosen
    finite    a candidate with a NaN or +-inf element scores +inf in every mode, and the medoid sums of the others leave it out
    choice    the smallest score, a non-finite one counting as +inf, ties to the lowest index
    spread    the population standard deviation over s, per element"""
from __future__ import annotations

import functools

import numpy as np

import flow_util as fu

SELECTS = ("first", "medoid", "coherent")


# ------------------------------------------------------------------------------------------------------------------ float64 reference
def _medoid_scores(x, good):
    with np.errstate(all="ignore"):
        d = x[:, None] - x[None, :]                       # (S, S', B, da)
        return np.where(good[None], (d * d).sum(-1), 0.0).sum(1).T      # (B, S): the sum over the finite s'


def _coherent_scores(x, prev, shift, K, w):
    S, B, da = x.shape
    A = da // K
    live = K - shift
    keep = np.asarray(w[:max(live, 0)]) != 0
    if live <= 0 or not keep.any():
        return np.zeros((B, S), dtype=x.dtype)
    with np.errstate(all="ignore"):
        xs = x.reshape(S, B, K, A)[:, :, :live][:, :, keep]
        y = prev.reshape(B, K, A)[:, shift:][:, keep]
        return (((xs - y[None]) ** 2).sum(-1) @ np.asarray(w[:live], dtype=x.dtype)[keep]).T      # (B, S)


def scores_ref(cand, select, prev=None, shift=0, K=1, w=None, row_mask=None, dtype=np.float64):
    """(B, S): the scores the choice is made from, non-finite ones as +inf"""
    x = np.asarray(cand, dtype=dtype)
    S, B, _ = x.shape
    good = np.isfinite(x).all(-1)                         # (S, B): a candidate with a NaN or +-inf element never wins
    sc = _medoid_scores(x, good)
    if select == "coherent":
        co = _coherent_scores(x, np.asarray(prev, dtype=dtype), shift, K, np.asarray(w, dtype=dtype))
        rows = np.ones(B, bool) if row_mask is None else np.asarray(row_mask) != 0
        sc = np.where(rows[:, None], co, sc)
    return np.where(np.isfinite(sc) & good.T, sc, np.inf)


def choice_of(scores) -> np.ndarray:
    """(B,) int32: np.argmin returns the FIRST smallest entry, and an all-inf row gives 0"""
    return np.argmin(scores, axis=1).astype(np.int32)


def select_ref(cand, select, **kw):
    """-> (scores (B, S) float64, choice (B) int32, spread (B, da) float64)"""
    sc = scores_ref(cand, select, **kw)
    ch = choice_of(sc) if select != "first" else np.zeros(sc.shape[0], np.int32)
    with np.errstate(all="ignore"):
        spread = np.asarray(cand, np.float64).std(axis=0)
    return sc, ch, spread


def runner_up_gap(scores) -> np.ndarray:
    """(B,): second smallest - smallest score of a row (inf with one candidate or one finite score; nan -> 0 when none is finite)"""
    if scores.shape[1] < 2:
        return np.full(scores.shape[0], np.inf)
    s = np.sort(scores, axis=1)
    with np.errstate(all="ignore"):
        return np.nan_to_num(s[:, 1] - s[:, 0], nan=0.0, posinf=np.inf)


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation of the kernel's sums
def _wave_sum32(lanes):
    """(..., 64) float32 -> (...): the xor butterfly of wave_sum, offsets 32, 16, .., 1"""
    v = lanes.astype(np.float32)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., idx ^ o]).astype(np.float32)
    return v[..., 0]


def _lane_sums32(terms):
    """(..., n) float32 terms -> (..., 64): lane l adds elements l, l + 64, .. in ascending order"""
    n = terms.shape[-1]
    pad = (-n) % 64
    t = np.concatenate([terms, np.zeros(terms.shape[:-1] + (pad,), np.float32)], axis=-1).reshape(terms.shape[:-1] + (-1, 64))
    acc = np.zeros(terms.shape[:-1] + (64,), np.float32)
    for r in range(t.shape[-2]):
        acc = (acc + t[..., r, :]).astype(np.float32)
    return acc


def select_emu32(cand, select, prev=None, shift=0, K=1, w=None, row_mask=None):
    """the selection kernel's arithmetic in fp32 on the CPU, in its order (lane-strided partial sums, one butterfly per pair / candidate, ascending folds;
    products and sums rounded separately) -> (scores (B, S), spread (B, da)).  Finite inputs only."""
    x = np.asarray(cand, np.float32)
    S, B, da = x.shape
    D = np.zeros((B, S, S), np.float32)
    for i in range(S):
        for j in range(i + 1, S):
            df = (x[i] - x[j]).astype(np.float32)
            D[:, i, j] = D[:, j, i] = _wave_sum32(_lane_sums32((df * df).astype(np.float32)))
    sc = np.zeros((B, S), np.float32)
    for s2 in range(S):
        sc = (sc + D[:, :, s2]).astype(np.float32)
    if select == "coherent":
        A = da // K
        live = (K - shift) * A
        w32 = np.repeat(np.asarray(w, np.float32), A)[:live]
        y = np.asarray(prev, np.float32)[:, shift * A:shift * A + live]
        co = np.zeros((B, S), np.float32)
        for s in range(S):
            df = (x[s][:, :live] - y).astype(np.float32)
            co[:, s] = _wave_sum32(_lane_sums32((w32 * (df * df).astype(np.float32)).astype(np.float32))) if live else 0.0
        rows = np.ones(B, bool) if row_mask is None else np.asarray(row_mask) != 0
        sc = np.where(rows[:, None], co, sc)
    s1 = np.zeros((B, da), np.float32)
    for s in range(S):
        s1 = (s1 + x[s]).astype(np.float32)
    mean = (s1 / np.float32(S)).astype(np.float32)
    q = np.zeros((B, da), np.float32)
    for s in range(S):
        df = (x[s] - mean).astype(np.float32)
        q = (q + (df * df).astype(np.float32)).astype(np.float32)
    return sc, np.sqrt((q / np.float32(S)).astype(np.float32)).astype(np.float32)


def rel_dist(got, ref) -> float:
    """max |got - ref| over the entries where ref is finite, relative to the largest finite |ref| (0 when ref is all 0)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    scale = np.abs(ref[fin]).max() if fin.any() else 0.0
    return float(np.abs(got[fin] - ref[fin]).max() / scale) if scale > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------------ the selection cases host and GPU tests share
# (K, A): tests/flow_util.py's heads -- awkward: da = 21, below one wave and no multiple of 4; larger: da = 700
HEADS = {"awkward": (3, 7), "larger": (50, 14)}
RANDOM_CASES = [(n, B, S) for n in HEADS for B in (1, 9) for S in (2, 5, 16)] + [("awkward", 67, 3), ("larger", 67, 3)]
SHIFTS = lambda K: (0, 1, K - 1, K)      # noqa: E731
DECAY = 0.5
NEAR_TIE_CAP = 0.05                      # the share of rows whose float64 runner-up may lie within the bar


def weights(K: int, decay: float = DECAY) -> np.ndarray:
    return np.array([decay ** k for k in range(K)], np.float32)


@functools.lru_cache(maxsize=None)
def random_case(name: str, B: int, S: int, seed: int = 0) -> dict:
    """candidates ~ N(0, 1) around a per-observation centre, prev near one of them, a row mask with zeros in it (B > 1), dataset statistics"""
    K, A = HEADS[name]
    da = K * A
    g = np.random.default_rng(4000 + seed + 31 * B + 7 * S + (0 if name == "awkward" else 500))
    cand = (g.standard_normal((1, B, da)) + g.standard_normal((S, B, da))).astype(np.float32)
    prev = (cand[g.integers(0, S, B), np.arange(B)] + 0.5 * g.standard_normal((B, da))).astype(np.float32)
    mask = np.ones(B, np.int32)
    mask[2::4] = 0
    return {"K": K, "A": A, "cand": cand, "prev": prev, "row_mask": mask, "w": weights(K), "shift": K // 3,
            "std": (g.random(da) + 0.5).astype(np.float32), "mean": g.standard_normal(da).astype(np.float32)}


def case_kwargs(c: dict, select: str, shift=None, masked: bool = True) -> dict:
    if select != "coherent":
        return {}
    return dict(prev=c["prev"], shift=c["shift"] if shift is None else shift, K=c["K"], w=c["w"], row_mask=c["row_mask"] if masked else None)


@functools.lru_cache(maxsize=None)
def emulation_distance(name: str, select: str):
    """-> (scores, spread): the fp32 emulation's distance from float64 (rel_dist) on this head's random cases, the largest over them.  One figure per head
    and score, not per case: a case with B = 1 and S = 2 has ONE distinct medoid score, and one sample of a rounding error says little about its size."""
    ds = dp = 0.0
    for n, B, S in RANDOM_CASES:
        if n != name:
            continue
        c = random_case(n, B, S)
        kw = case_kwargs(c, select)
        sc64, _, sp64 = select_ref(c["cand"], select, **kw)
        sc32, sp32 = select_emu32(c["cand"], select, **kw)
        ds, dp = max(ds, rel_dist(sc32, sc64)), max(dp, rel_dist(sp32, sp64))
    return ds, dp


def decided_rows(scores64, bar: float) -> np.ndarray:
    """(B,) bool: rows whose float64 runner-up lies more than `bar` (relative to the largest finite score of the case) above the winner"""
    fin = np.isfinite(scores64)
    scale = np.abs(scores64[fin]).max() if fin.any() else 1.0
    return runner_up_gap(scores64) > bar * scale


@functools.lru_cache(maxsize=None)
def exact_case(name: str, B: int, S: int) -> dict:
    """small-integer candidates, prev and weights: every difference, square, product and partial sum is an integer below 2^24, so fp32 sums are exact in any
    order.  Candidate S - 1 is a copy of candidate 0 of every row (a duplicate pair ties; the lower index must win when it is the best)."""
    K, A = HEADS[name]
    da = K * A
    g = np.random.default_rng(77 + 3 * B + S + (0 if name == "awkward" else 9))
    cand = g.integers(-3, 4, (S, B, da)).astype(np.float32)
    if S > 1:
        cand[S - 1] = cand[0]
    prev = g.integers(-3, 4, (B, da)).astype(np.float32)
    if S > 1:
        prev[::2] = cand[0, ::2]                     # every other row: candidates 0 and S - 1 both score 0 over any overlap
    mask = np.ones(B, np.int32)
    mask[1::3] = 0
    return {"K": K, "A": A, "cand": cand, "prev": prev, "row_mask": mask, "w": np.array([(2, 1, 0)[k % 3] for k in range(K)], np.float32), "shift": K // 3,
            "std": np.full(da, 2.0, np.float32), "mean": np.full(da, -1.0, np.float32)}


# ------------------------------------------------------------------------------------------------------------------ the two-mode toy
def toy_field(x, t):
    """the exact velocity field of the target whose chunks are wholly +1 or wholly -1 (each with probability 1 / 2), x (.., D), 0 < t <= 1"""
    return (x - np.tanh((1.0 - t) * x.sum(-1, keepdims=True) / (t * t))) / t


def toy_sample(noise, N: int = 10):
    """float64 Euler from t = 1 to 0 in N steps"""
    x = np.asarray(noise, np.float64).copy()
    for i in range(N):
        x = x - toy_field(x, 1.0 - i / N) / N
    return x


def toy_figures(obs: int = 512, S: int = 8, D: int = 4, N: int = 10, seed: int = 0) -> dict:
    """`obs` observations x S candidates: how often one sample / the candidate nearest a previous all-+ chunk lands in the + mode, and mean |x| of the medoid and
    of the mean of the candidates"""
    x = toy_sample(np.random.default_rng(seed).standard_normal((obs, S, D)), N)
    cand = np.ascontiguousarray(x.transpose(1, 0, 2))                              # (S, obs, D)
    prev = np.ones((obs, D))
    _, coh, _ = select_ref(cand, "coherent", prev=prev, shift=0, K=1, w=np.ones(1))
    _, med, _ = select_ref(cand, "medoid")
    rows = np.arange(obs)
    return {"single_plus": float((cand[0].mean(-1) > 0).mean()), "coherent_plus": float((cand[coh, rows].mean(-1) > 0).mean()),
            "rows_without_plus": int(((cand.mean(-1) > 0).sum(0) == 0).sum()), "medoid_mean_abs": float(np.abs(cand[med, rows]).mean()),
            "mean_mean_abs": float(np.abs(cand.mean(0)).mean())}
