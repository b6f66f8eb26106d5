"""The EMA update of the fused step (csrc/common.h ema_update) restated in float64, and its bound.

    e' = e + w (p_new - e)            from the device's own float32 p_new, e_old and w

The kernel rounds twice: the difference p_new - e (half a spacing of it: at most 2^-24 |p_new - e|, which the product with w scales) and the fma (half a
spacing of the result).  The bound is TWICE that sum, derived and not measured:

    |e - e64| <= spacing_fp32(|e64|) + 2^-23 w |p_new - e_old|

w == 1 must give p_new and w == 0 must leave e alone, both bit for bit; those are asserted separately."""
import numpy as np
import torch


def ema_ref(e_old: torch.Tensor, p_new: torch.Tensor, w: float) -> torch.Tensor:
    """float32 CPU tensors and the float32 weight -> e64"""
    w = float(np.float32(w))
    e, p = e_old.double(), p_new.double()
    return e + w * (p - e)


def ema_bound(e64: torch.Tensor, e_old: torch.Tensor, p_new: torch.Tensor, w: float) -> torch.Tensor:
    sp = torch.from_numpy(np.spacing(np.abs(e64.numpy()).astype(np.float32)).astype(np.float64))
    return sp + 2.0 ** -23 * float(np.float32(w)) * (p_new.double() - e_old.double()).abs()


def check_ema(what: str, e_new: torch.Tensor, e_old: torch.Tensor, p_new: torch.Tensor, w: float) -> float:
    """asserts the bound for every element; -> the worst error / bound (printed: a figure to read beside the assertion)"""
    e_new, e_old, p_new = (t.detach().cpu().reshape(-1) for t in (e_new, e_old, p_new))
    e64 = ema_ref(e_old, p_new, w)
    err, bound = (e_new.double() - e64).abs(), ema_bound(e64, e_old, p_new, w)
    worst = float((err / bound).max())
    print(f"[{what}] w = {float(np.float32(w))!r}: ema error / bound {worst:.3f} over {e_new.numel()} elements")
    if not bool((err <= bound).all()):
        i = int((err / bound).argmax())
        print(f"[{what}] worst element {i}: e_old {float(e_old[i])!r} p_new {float(p_new[i])!r} e64 {float(e64[i])!r} e {float(e_new[i])!r} bound {float(bound[i]):.3e}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements outside spacing + 2^-23 w |p - e|, worst {worst:.2f} x the bound"
    if float(np.float32(w)) == 1.0:
        assert torch.equal(e_new, p_new), f"{what}: w = 1 must copy p_new bit for bit"
    if float(np.float32(w)) == 0.0:
        assert torch.equal(e_new, e_old), f"{what}: w = 0 must leave the average alone"
    return worst
