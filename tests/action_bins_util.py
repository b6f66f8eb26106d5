"""float64 evaluation of the binned action head (include/fastvla_hip.h, "binned action head"): the reference the action-bins tests compare against, written
from the formulas alone.

Logits z are (B, K, A, Nb); a group is the Nb logits of one action element.  Element (k, a) of a row -- e = k A + a -- has the range [lo, hi] = pair e % R of the R
given pairs.  w = fp32((hi - lo) / Nb) (formed in double, rounded once: the number the library uploads); bin j covers [lo + j w, lo + (j + 1) w), its centre is
lo + (j + 1/2) w, the last edge is hi itself.  A target is clamped to [lo, hi]; its bin is min(Nb - 1, floor((a - lo) / w)).
    sigma == 0: q one-hot at the target's bin
    sigma > 0:  q_j = [Phi((e_{j+1} - a) / S) - Phi((e_j - a) / S)] / [Phi((hi - a) / S) - Phi((lo - a) / S)],  S = sigma w
    loss = sum_valid om (-sum_j q_j log p_j) / n        g_j = loss_scale om (p_j - q_j) / n        n = B K A, om = dim_w[a] step_w[k] (1 without weights)
A padded step or an om == 0 element is selected away: whatever its target holds it contributes exactly 0.
metrics = (sum over valid, om != 0 elements of (decoded - target)^2 / n, valid steps / (B K), hits / valid elements): unweighted, valid looks at pads only."""
import numpy as np
import torch

SQRT1_2 = 0.70710678118654752440


def bins_table(ranges, nb, da):
    """ranges: a list of R (lo, hi) pairs, R dividing da -> (lo, hi, w) fp32 arrays of R entries, w = fp32((hi - lo) / nb) from double"""
    pairs = [tuple(ranges)] if len(ranges) == 2 and not hasattr(ranges[0], "__len__") else [tuple(p) for p in ranges]
    assert da % len(pairs) == 0
    lo = np.array([p[0] for p in pairs], dtype=np.float32)
    hi = np.array([p[1] for p in pairs], dtype=np.float32)
    w = ((hi.astype(np.float64) - lo.astype(np.float64)) / nb).astype(np.float32)
    return lo, hi, w


def per_element(table, K, A):
    """(lo, hi, w) of R entries -> three float64 (K, A) arrays: element e = k A + a reads entry e % R"""
    e = np.arange(K * A)
    return tuple(np.asarray(v, dtype=np.float64)[e % len(v)].reshape(K, A) for v in table)


def phi_diff(x1, x2):
    """Phi(x2) - Phi(x1), x1 <= x2, float64 tensors: through erfc on the side where both tails are small"""
    up = 0.5 * (torch.special.erfc(x1 * SQRT1_2) - torch.special.erfc(x2 * SQRT1_2))
    dn = 0.5 * (torch.special.erfc(-x2 * SQRT1_2) - torch.special.erfc(-x1 * SQRT1_2))
    return torch.where(x1 > 0, up, dn)


def target_index(t, lo, hi, w, nb):
    """t, lo, hi, w broadcastable float64 arrays -> (clamped target, bin index)"""
    a = np.clip(t, lo, hi)
    return a, np.minimum(nb - 1, np.floor((a - lo) / w)).astype(np.int64)


def target_dist(t, lo, hi, w, nb, sigma):
    """-> q (..., nb) float64 for targets t (...) with per-element lo, hi, w (...)"""
    t, lo, hi, w = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(t, lo, hi, w))
    a, idx = target_index(t, lo, hi, w, nb)
    if sigma == 0:
        q = np.zeros(t.shape + (nb,))
        np.put_along_axis(q, idx[..., None], 1.0, axis=-1)
        return q
    j = np.arange(nb + 1, dtype=np.float64)
    edges = lo[..., None] + j * w[..., None]
    edges[..., nb] = hi                                             # the last edge is hi itself
    x = torch.from_numpy((edges - a[..., None]) / (sigma * w[..., None]))
    num = phi_diff(x[..., :-1], x[..., 1:])
    den = phi_diff(x[..., :1], x[..., -1:])
    return (num / den).numpy()


def decode_ref(z, lo, w, mode):
    """z (..., nb) float64 logits -> decoded values (...): "argmax" the centre of the first largest logit, "mean" sum_j softmax(z)_j c_j"""
    nb = z.shape[-1]
    c = lo[..., None] + (np.arange(nb) + 0.5) * w[..., None]
    if mode == "argmax":
        return np.take_along_axis(c, np.argmax(z, axis=-1)[..., None], axis=-1)[..., 0]
    p = torch.softmax(torch.from_numpy(z), dim=-1).numpy()
    return (p * c).sum(-1)


def bins_ref(z, t, table, pad=None, sigma=0.0, decode="argmax", dim_w=None, step_w=None, loss_scale=1.0):
    """z (B, K, A, Nb), t (B, K, A) array-likes; table = bins_table(...); pad (B, K) bool or None; dim_w (A) / step_w (K) or None ->
    dict(loss, g (B, K, A, Nb), om (K, A), live (B, K, A) bool, sqerr, valid, acc, decoded (B, K, A), idx, p) in float64"""
    z = np.asarray(z, dtype=np.float64)
    B, K, A, nb = z.shape
    n = B * K * A
    lo, hi, w = per_element(table, K, A)
    valid = np.ones((B, K), dtype=bool) if pad is None else ~np.asarray(pad, dtype=bool).reshape(B, K)
    om = np.ones((K, A)) if dim_w is None else np.asarray(step_w, dtype=np.float64)[:, None] * np.asarray(dim_w, dtype=np.float64)[None, :]
    live = valid[:, :, None] & (om != 0)[None]
    ts = np.where(live, np.asarray(t, dtype=np.float64), 0.0)        # select: a masked target never enters the arithmetic
    q = target_dist(ts, lo[None], hi[None], w[None], nb, sigma)
    zt = torch.from_numpy(z)
    logp, p = torch.log_softmax(zt, dim=-1).numpy(), torch.softmax(zt, dim=-1).numpy()
    ce = -(np.where(q > 0, q * logp, 0.0)).sum(-1)
    loss = float(np.where(live, om[None] * ce, 0.0).sum() / n)
    g = np.where(live[..., None], loss_scale * om[None, :, :, None] * (p - q) / n, 0.0)
    dec = decode_ref(z, np.broadcast_to(lo[None], (B, K, A)), np.broadcast_to(w[None], (B, K, A)), decode)
    _, idx = target_index(ts, lo[None], hi[None], w[None], nb)
    d = np.where(live, dec - ts, 0.0)
    hits = (np.argmax(z, axis=-1) == idx) & live
    nvalid = int(valid.sum()) * A
    return {"loss": loss, "g": g, "om": om, "live": live, "sqerr": float((d * d).sum() / n), "abs_d": np.abs(d), "valid": float(valid.sum() / (B * K)),
            "acc": float(hits.sum() / nvalid) if nvalid else 0.0, "nvalid": nvalid, "hits": int(hits.sum()), "decoded": dec, "idx": idx, "p": p}


def torch_bins_loss(logits, t, table, pad=None, sigma=0.0, dim_w=None, step_w=None):
    """the same loss, differentiable in the float64 `logits` (B, K, A, Nb) tensor; t (B, K, A) tensor, pad (B, K) bool tensor or None"""
    B, K, A, nb = logits.shape
    lo, hi, w = per_element(table, K, A)
    valid = torch.ones(B, K, dtype=torch.bool) if pad is None else ~pad.reshape(B, K)
    om = np.ones((K, A)) if dim_w is None else np.asarray(step_w, dtype=np.float64)[:, None] * np.asarray(dim_w, dtype=np.float64)[None, :]
    live = valid[:, :, None] & torch.from_numpy(om != 0)[None]
    ts = np.where(live.numpy(), t.detach().double().numpy(), 0.0)
    q = torch.from_numpy(target_dist(ts, lo[None], hi[None], w[None], nb, sigma))
    ce = -(q * torch.log_softmax(logits, dim=-1)).sum(-1)
    return torch.where(live, torch.from_numpy(om)[None] * ce, torch.zeros_like(ce)).sum() / (B * K * A)


def make_targets(B, K, A, table, nb, seed, margin=1e-3):
    """targets (B, K, A) fp32 in [lo - 0.2 span, hi + 0.2 span] (the clamp is exercised), every one at least margin * w away from any bin edge -- in range from
    the edges of its bin, out of range from lo and hi -- so that the bin of a hard target is the same in fp32 and float64.  The condition is asserted here."""
    g = torch.Generator().manual_seed(seed)
    lo, hi, w = per_element(table, K, A)
    span = hi - lo
    u = torch.rand(B, K, A, generator=g, dtype=torch.float64).numpy()
    t = (lo - 0.2 * span)[None] + 1.4 * span[None] * u
    pos = (t - lo[None]) / w[None]
    frac = pos - np.floor(pos)
    near = (frac < 4 * margin) | (frac > 1 - 4 * margin)
    t = np.where(near, lo[None] + (np.floor(pos) + 0.5) * w[None], t)
    t32 = t.astype(np.float32)
    pos = (t32.astype(np.float64) - lo[None]) / w[None]
    frac = pos - np.floor(pos)
    assert bool(((frac >= margin) & (frac <= 1 - margin)).all()), "a target lies within margin * w of a bin edge"
    assert bool((t32 < lo[None]).any() and (t32 > hi[None]).any()) or B * K * A < 8
    return torch.from_numpy(t32)
