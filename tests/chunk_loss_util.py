"""float64 evaluation of the chunked action loss (include/fastvla_hip.h, fv_head_set_loss): the reference the action-chunk tests compare against.

With d = a - t over (B, K, A), n = B K A and w = 0 where pad[b][k] else 1:
    loss = sum w rho(d) / n        g = loss_scale w rho'(d) / n        metrics = (sum w d^2 / n, valid steps / (B K))
rho: mse d^2; l1 |d| with sign(0) = 0; smooth_l1 0.5 d^2 / beta for |d| < beta, else |d| - 0.5 beta.  The denominator is ALL n elements.  A padded element
is selected away, so whatever its target holds (NaN, +-inf) it contributes exactly 0."""
import numpy as np
import torch

KINDS = ("mse", "l1", "smooth_l1")


def chunk_loss_ref(a, t, pad=None, kind="mse", beta=1.0, loss_scale=1.0):
    """a, t: (B, K, A) array-likes; pad: (B, K) bool or None -> dict(loss, mse, valid, g (B, K, A)) in float64"""
    a, t = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)
    assert a.ndim == 3 and a.shape == t.shape
    B, K, A = a.shape
    n = a.size
    w = np.ones((B, K), dtype=bool) if pad is None else ~np.asarray(pad, dtype=bool).reshape(B, K)
    we = np.broadcast_to(w[:, :, None], a.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(we, a - np.where(we, t, 0.0), 0.0)      # select: a padded target never enters the arithmetic
    ad = np.abs(d)
    if kind == "mse":
        rho, drho = d * d, 2.0 * d
    elif kind == "l1":
        rho, drho = ad, np.sign(d)
    elif kind == "smooth_l1":
        rho = np.where(ad < beta, 0.5 * d * d / beta, ad - 0.5 * beta)
        drho = np.where(ad < beta, d / beta, np.sign(d))
    else:
        raise ValueError(kind)
    rho, drho = np.where(we, rho, 0.0), np.where(we, drho, 0.0)
    return {"loss": float(rho.sum() / n), "mse": float(np.where(we, d * d, 0.0).sum() / n), "valid": float(w.sum() / (B * K)), "g": loss_scale * drho / n}


def torch_loss_ref(a, t, pad=None, kind="mse", beta=1.0):
    """the same loss the way a LeRobot policy spells it: torch's elementwise loss, times the mask, .mean() -- float64, differentiable in a"""
    import torch.nn.functional as F
    fn = {"mse": F.mse_loss, "l1": F.l1_loss, "smooth_l1": lambda x, y, reduction: F.smooth_l1_loss(x, y, reduction=reduction, beta=beta)}[kind]
    per = fn(a, t, reduction="none")
    if pad is not None:
        per = torch.where(pad.unsqueeze(-1).expand_as(per), torch.zeros_like(per), per)
    return per.sum() / per.numel()


def ragged_pad(B, K, seed=0):
    """a trailing run of padded steps per row (what LeRobot's action_is_pad looks like near an episode end): lengths cycle through 0 .. K, so both an
    all-valid and an all-padded row occur once B > K"""
    pad = np.zeros((B, K), dtype=bool)
    for b in range(B):
        k = (b + seed) % (K + 1)
        if k:
            pad[b, K - k:] = True
    return pad
