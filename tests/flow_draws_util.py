"""Float64 reference of a flow-head step with S noise draws per observation (fv_head_set_flow_draws; tests only).

Head rows are draw-major, r = s B + b.  The conditioning (pooled feature, state) is ONE leaf per observation that every draw reads through autograd, so the
reference sums d_pooled over the draws by itself.  The loss is sum over all S B K A elements of w rho(d) / (S B K A): the mean of the S single-draw losses."""
from __future__ import annotations

import numpy as np
import torch

import flow_util as fu

HEADS = ("awkward", "larger")
BATCHES, DRAWS = (1, 9), (1, 2, 5, 8)


def loss_ref(pred, u, pad, kind, dim_w=None, step_w=None):
    """pred, u: (R, K, A) float64 torch; pad: (R, K) bool torch or None -> sum w rho(d) / numel, differentiable in pred.  A padded or zero-weight element is
    selected away."""
    d = pred - u
    rho = d * d if kind == "mse" else d.abs()
    if dim_w is not None or step_w is not None:
        K, A = pred.shape[1], pred.shape[2]
        om = (torch.ones(K, dtype=torch.float64) if step_w is None else step_w.double()).view(1, K, 1) * \
             (torch.ones(A, dtype=torch.float64) if dim_w is None else dim_w.double()).view(1, 1, A)
        rho = torch.where((om == 0).expand_as(rho), torch.zeros_like(rho), rho * om)
    if pad is not None:
        rho = torch.where(pad.unsqueeze(-1).expand_as(rho), torch.zeros_like(rho), rho)
    return rho.sum() / rho.numel()


def draws_reference(p: dict, pooled, states, a, eps, t, pad, kind: str, S: int, dims, dim_w=None, step_w=None, rows=None) -> dict:
    """p: the head's tensors; pooled (B, feat), states (B, ds), a (B, da): per observation; eps (S B, da), t (S B): per head row, draw-major; pad (B, K) bool
    numpy or None.  rows: the draws to take (default all S; the reference of ONE single-draw call is rows = [s]).
    -> {"loss", "pred" (len(rows) B, da), "grads": {name: tensor}, "d_pooled" (B, feat)}, all float64"""
    feat, ds, hid, fus, K, A, E = dims
    B, da = a.shape[0], K * A
    rows = list(range(S)) if rows is None else list(rows)
    n = len(rows)
    pick = torch.cat([torch.arange(s * B, (s + 1) * B) for s in rows])
    eps, t = torch.as_tensor(eps)[pick], torch.as_tensor(t)[pick]
    p64 = {k: w.detach().double().requires_grad_(True) for k, w in p.items()}
    pooled64 = pooled.detach().double().requires_grad_(True)
    x_ref, u_ref = fu.noising_ref(np.tile(a.numpy(), (n, 1)), eps.numpy(), t.numpy())
    phi = fu.phi_ref(t.numpy(), fu.flow_freqs(E))
    pred = fu.velocity(p64, pooled64.repeat(n, 1), states.double().repeat(n, 1), torch.from_numpy(x_ref), torch.from_numpy(phi))
    padt = None if pad is None else torch.from_numpy(np.tile(np.asarray(pad, dtype=bool), (n, 1)))
    loss = loss_ref(pred.view(n * B, K, A), torch.from_numpy(u_ref).view(n * B, K, A), padt, kind, dim_w, step_w)
    loss.backward()
    return {"loss": loss.detach(), "pred": pred.detach(), "grads": {k: w.grad for k, w in p64.items()}, "d_pooled": pooled64.grad}


def mean_of_singles(p, pooled, states, a, eps, t, pad, kind, S, dims, dim_w=None, step_w=None) -> dict:
    """the mean of the S single-draw references, each one a call of draws_reference on its own draw: what the S-draw step is defined to equal"""
    one = [draws_reference(p, pooled, states, a, eps, t, pad, kind, S, dims, dim_w, step_w, rows=[s]) for s in range(S)]
    return {"loss": sum(r["loss"] for r in one) / S, "grads": {k: sum(r["grads"][k] for r in one) / S for k in one[0]["grads"]},
            "d_pooled": sum(r["d_pooled"] for r in one) / S, "d_pooled_each": [r["d_pooled"] for r in one], "each": one}


def case(name: str, B: int, S: int, seed: int = 0) -> dict:
    """one head-step case: parameters, observation, targets, per-row noise and time"""
    feat, ds, hid, fus, K, A, E = fu.DIMS[name]
    da = K * A
    p = fu.flow_head_params(fu.flow_head_shapes(feat, ds, da, hid, fus, E), 7, scale=0.2 if name == "awkward" else 0.05)
    g = torch.Generator().manual_seed(80 + seed + 3 * B + 11 * S)
    return {"dims": fu.DIMS[name], "p": p, "pooled": torch.randn(B, feat, generator=g), "states": torch.randn(B, ds, generator=g),
            "a": torch.randn(B, da, generator=g), "eps": torch.randn(S * B, da, generator=g), "t": torch.rand(S * B, generator=g)}


def train_offset(rank: int, step: int, micro: int) -> int:
    """the host's offset layout of a train step (FastVLMWithExpert.flow_train_draw): micro bits 0 .. 15, step 16 .. 43, rank from 44 up"""
    return (int(rank) << 44) + (int(step) << 16) + (int(micro) & 0xFFFF)
