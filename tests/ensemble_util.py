"""float64 references of temporal ensembling (include/fastvla_hip.h, fv_ensemble_step; LeRobot's ACTTemporalEnsembler per environment), in two independent
forms the host test holds against each other:

  * `ensemble_online`: the online update LeRobot runs -- a buffer of K running means that is shifted by one every step (no ring), a count per entry,
    ens <- (ens cumsum_w[n-1] + c w[n]) / cumsum_w[n];
  * `ensemble_closed`: the definition -- every chunk since the last reset is stored with the step it was predicted at, and the action of step t is
    sum_i w_i c_i[t] / sum_i w_i over the stored chunks that reach t, i = 0 the OLDEST of them, w_i = exp(-coeff i).

chunks: (T, n_env, K, A), the chunk every environment predicts at steps 0 .. T-1.  resets: {step: [env, ...]} -- environment env forgets its history
BEFORE the update of that step (None in the list = all).  -> (T, n_env, A) float64.  `ensemble_online_fp32` is the online form again with every operation
rounded to fp32, tables included: what the derived error bar of the GPU test is checked against on the host."""
import math

import numpy as np


def weights(coeff, K):
    w = np.array([math.exp(-float(coeff) * i) for i in range(K)], dtype=np.float64)
    return w, np.cumsum(w)


def _reset_envs(resets, t, n_env):
    envs = (resets or {}).get(t, [])
    return list(range(n_env)) if any(e is None for e in envs) else list(envs)


def ensemble_online(chunks, coeff, resets=None, dtype=np.float64):
    chunks = np.asarray(chunks, dtype=dtype)
    T, n_env, K, A = chunks.shape
    w, cw = (x.astype(dtype) for x in weights(coeff, K))
    out = np.zeros((T, n_env, A), dtype=dtype)
    buf = [None] * n_env            # per environment: (means (m, A), counts (m,)) for the m <= K time steps from now on that have a prediction
    for t in range(T):
        for e in _reset_envs(resets, t, n_env):
            buf[e] = None
        for e in range(n_env):
            c = chunks[t, e]
            if buf[e] is None:
                means, counts = c.copy(), np.ones(K, dtype=np.int64)
            else:
                means, counts = buf[e]
                m = means.shape[0]                      # K - 1 entries carried over: the new chunk's rows 0 .. m-1 update them, row m .. K-1 are new
                upd = np.empty_like(means)
                for k in range(m):
                    n = counts[k]
                    upd[k] = ((means[k] * cw[n - 1]).astype(dtype) + (c[k] * w[n]).astype(dtype)).astype(dtype) / cw[n]
                means = np.concatenate([upd, c[m:]], axis=0).astype(dtype)
                counts = np.concatenate([np.minimum(counts + 1, K), np.ones(K - m, dtype=np.int64)])
            out[t, e] = means[0]
            buf[e] = (means[1:], counts[1:]) if K > 1 else None
    return out


def ensemble_online_fp32(chunks, coeff, resets=None):
    return ensemble_online(chunks, coeff, resets, dtype=np.float32)


def ensemble_closed(chunks, coeff, resets=None):
    chunks = np.asarray(chunks, dtype=np.float64)
    T, n_env, K, A = chunks.shape
    w, _ = weights(coeff, K)
    out = np.zeros((T, n_env, A))
    since = np.zeros(n_env, dtype=np.int64)             # the first step whose chunk still counts, per environment
    for t in range(T):
        for e in _reset_envs(resets, t, n_env):
            since[e] = t
        oldest = np.maximum(since, t - K + 1)           # per environment: the oldest stored chunk that reaches t; it carries w[0]
        num, den = np.zeros((n_env, A)), np.zeros(n_env)
        for t0 in range(max(0, t - K + 1), t + 1):      # oldest first
            has = t0 >= oldest
            wi = np.where(has, w[np.clip(t0 - oldest, 0, K - 1)], 0.0)
            num += np.where(has[:, None], wi[:, None] * chunks[t0, :, t - t0], 0.0)      # (selected, not multiplied: a NaN in a chunk that does not count stays out)
            den += wi
        out[t] = num / den[:, None]
    return out


def error_bar(K, max_abs):
    """the GPU tests' bar per served element: 6 K 2^-24 max|chunk|.  Per online update two products, one sum, one quotient and two rounded table entries
    (six roundings of relative size 2^-24 at the most); a slot sees at most K - 1 updates; every value is a convex combination of chunk values, hence
    bounded by max|chunk|."""
    return 6.0 * K * 2.0 ** -24 * max_abs
