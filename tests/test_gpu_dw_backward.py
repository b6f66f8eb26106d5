"""-m gpu: every kernel instance of the depthwise convs' backward, each on its own entry point, against exact or float64 references (tests/dw_bwd_util.py).

  fv_op_dw_dgrad       dw_dgrad_kernel<k, stride, mult>, the five instances (3,1,1) (7,1,1) (3,2,1) (7,2,2) (3,1,2)
  fv_op_dw_dgrad_mfma  dwconv_march_kernel<3 | 7, GRAD>, the route the tower's backward takes for stride-1 maps with C % 32 == 0, W >= 16, H >= 16
  fv_op_dw_wgrad       dw_wgrad_mfma_kernel<7>, dw_wgrad_lds_kernel, dw_wgrad_rows_kernel, dw_wgrad_kernel (the last three in the five instances)

Every case asserts the route it was written for against the route mirror (dw_bwd_util.*_route), so a case cannot drift to another kernel unnoticed; the CPU file
tests/test_dw_backward_reference_host.py checks that the tables cover every reachable (route x instance) pair.

EXACT class: x, dy integers in [-4, 4], taps in [-3, 3], res in [-512, 512].  Every product and partial sum is an integer below 2^24 (exact in fp32 in any order),
every input-gradient result is below 2048 (exact in fp16): the kernels must give the int64 reference bit for bit, twice.  Outputs are pre-filled with NaN and carry
a NaN tail (one more row; for the partial-sum scratch, which is sized EXACTLY to dw_bwd_scratch_floats, 4096 floats) that must survive.

SELECTION: one non-zero dy element per channel, at the four corners / the last valid output position / an interior one: the input gradient is the flipped kernel
stamped there and clipped at the border, the tap gradient is the shifted x window with exact zeros where a tap falls outside the map.

SATURATION (both input-gradient routes; centre tap 2, all others 0, so conv^T(dy) = 2 dy): dy = +-60000 -> exactly +-65504, everything else exact, and *sat up by
exactly the number of (pixel, 8-channel group) cells holding a clamped value -- two clamped channels of one group are ONE cell, two groups of one pixel are two.
With a residual the two routes differ in ONE documented place:
  res pushes a finite sum over (conv 60000, res 6000): both routes clamp the sum and count the cell.
  res pulls a clamped conv back (conv 120000, res -60000): the VALU kernel sums in fp32 -- 60000, nothing clamps, nothing counts.  The MFMA kernel hands conv^T(dy)
  to the residual add through fp16 cells in LDS: the conv value itself is out of range there, so the cell is written as +65504 and counted once (it used to come
  out as 65504 - 60000 = 5504 with nothing counted).

ROUNDING class (Gaussian dy, taps, res; the reference in float64 on the same stored values), per element, A = sum |w dy|:
  VALU: |got - ref| <= 2^-11 |ref| + 2^-25 + 2 k^2 mult 2^-24 (A + |res|)     (one fp16 rounding of the result; fp32 products and sums)
  MFMA: the same plus a second 2^-11 |ref|                                     (the budget of a second fp16 rounding on the way to the residual add)
The bounds are derived, not measured.  The MFMA one found a defect: the kernel rounded conv^T(dy) ALONE to fp16 before the residual add, which leaves 2^-11 |conv| --
not |ref| -- in a sum that cancels (up to 134 times the bound on these inputs); it now carries the dropped part in a second LDS cell and rounds the sum once.  Each case prints its worst fraction of the bound (pytest -s shows it; docs/kernels.md records the MI355X figures)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dw_bwd_util as U  # noqa: E402
from gpu_util import DEV, call, check_close, lib, stream  # noqa: E402

NAN = float("nan")
FV_ERR_ARG, FV_ERR_UNSUPPORTED = -1, -5


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g)


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(v) for v in key)) % (2 ** 31))


def _dev16(t_nchw, dtype=torch.float16):
    return U.nhwc(t_nchw.to(torch.float32)).to(dtype).to(DEV)


def _out16(B, H, W, C):
    """NaN-filled fp16 output of B*H*W*C elements plus one more row of W*C: (whole buffer, the tail)"""
    buf = torch.full((B * H * W * C + W * C,), NAN, dtype=torch.float16, device=DEV)
    return buf, buf[B * H * W * C:]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def _dgrad(dy, w, res, Hi, Wi, k, stride, mult, *, round_w=0, mfma=False, flip=True, with_sat=True):
    """dy (B,Co,Ho,Wo) / res (B,Ci,Hi,Wi) CPU tensors of fp16-exact values, w tap-major [k*k][Co] fp32 -> (dx (B,Ci,Hi,Wi) fp16 on the CPU, *sat).  Runs the call twice
    into fresh NaN-filled buffers and requires identical bits, an untouched tail and the same count."""
    B, Co = dy.shape[0], dy.shape[1]
    Ci = Co // mult
    dyd = _dev16(dy)
    rd = None if res is None else _dev16(res)
    wd = U.toeplitz_flipped16(w, k, flip=flip).to(DEV).contiguous() if mfma else w.to(torch.float32).to(DEV).contiguous()
    outs = []
    for rep in range(2):
        buf, tail = _out16(B, Hi, Wi, Ci)
        sat = torch.zeros(4, dtype=torch.int32, device=DEV)
        sp = sat.data_ptr() if with_sat else None
        rp = None if rd is None else rd.data_ptr()
        if mfma:
            call(lib().fv_op_dw_dgrad_mfma(dyd.data_ptr(), wd.data_ptr(), rp, buf.data_ptr(), B, Hi, Wi, Ci, k, sp, stream()), "fv_op_dw_dgrad_mfma")
        else:
            call(lib().fv_op_dw_dgrad(dyd.data_ptr(), wd.data_ptr(), rp, buf.data_ptr(), B, Hi, Wi, Ci, k, stride, mult, round_w, sp, stream()), "fv_op_dw_dgrad")
        torch.cuda.synchronize()
        assert bool(torch.isnan(tail).all()), "the row behind the output was written"
        assert sat[1:].tolist() == [0, 0, 0]
        outs.append((buf[:B * Hi * Wi * Ci].cpu(), int(sat[0])))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and outs[0][1] == outs[1][1], "two runs differ"
    assert not bool(torch.isnan(outs[0][0]).any()), "an output element was not written (or is NaN)"
    return U.nchw(outs[0][0].view(B, Hi, Wi, Ci)), outs[0][1]


def _wgrad(x, dy, k, stride, mult, expect_route):
    """x (B,Ci,Hi,Wi) bf16-exact, dy (B,Co,Ho,Wo) fp16-exact -> (dw [k*k][Co], db [Co]) fp32 on the CPU.  Scratch sized exactly, NaN tail; twice, identical bits."""
    B, Ci, Hi, Wi = x.shape
    Co, Ho, Wo = dy.shape[1], dy.shape[2], dy.shape[3]
    assert U.wgrad_route(B, Hi, Wi, Ci, k, stride, mult) == expect_route
    nfl = U.wgrad_scratch_floats(B, Ho, Wo, Co, k)
    assert U.wgrad_part_rows(B, Hi, Wi, Ci, k, stride, mult) * (k * k + 1) * Co <= nfl      # checked on the CPU before anything is launched
    xd, dyd = _dev16(x, torch.bfloat16), _dev16(dy)
    outs = []
    for rep in range(2):
        scr = torch.full((nfl + 4096,), NAN, dtype=torch.float32, device=DEV)
        dw = torch.full((k * k * Co + Co,), NAN, dtype=torch.float32, device=DEV)
        db = torch.full((2 * Co,), NAN, dtype=torch.float32, device=DEV)
        call(lib().fv_op_dw_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), scr.data_ptr(), nfl, B, Hi, Wi, Ci, k, stride, mult, stream()), "fv_op_dw_wgrad")
        torch.cuda.synchronize()
        assert bool(torch.isnan(scr[nfl:]).all()), "partial sums written behind dw_bwd_scratch_floats"
        assert bool(torch.isnan(dw[k * k * Co:]).all()) and bool(torch.isnan(db[Co:]).all())
        outs.append((dw[:k * k * Co].cpu().view(k * k, Co), db[:Co].cpu()))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1])), "two runs differ"
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())
    # one element fewer than the launcher needs is refused before anything is enqueued
    assert lib().fv_op_dw_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), scr.data_ptr(), nfl - 1, B, Hi, Wi, Ci, k, stride, mult, stream()) == FV_ERR_ARG
    return outs[0]


def _exact_inputs(B, Ci, Hi, Wi, k, stride, mult, *key):
    g = _gen(k, stride, mult, Ci, Hi, Wi, *key)
    Co, Ho, Wo = Ci * mult, U.out_size(Hi, k, stride), U.out_size(Wi, k, stride)
    return (_ints((B, Ci, Hi, Wi), -4, 4, g), _ints((B, Co, Ho, Wo), -4, 4, g), _ints((k * k, Co), -3, 3, g), _ints((B, Ci, Hi, Wi), -512, 512, g))


def _gauss_inputs(B, Ci, Hi, Wi, k, stride, mult, *key):
    g = _gen(k, stride, mult, Ci, Hi, Wi, 77, *key)
    Co, Ho, Wo = Ci * mult, U.out_size(Hi, k, stride), U.out_size(Wi, k, stride)
    dy = (torch.randn(B, Co, Ho, Wo, generator=g) * 0.25).half()
    w = torch.randn(k * k, Co, generator=g) / k
    res = (torch.randn(B, Ci, Hi, Wi, generator=g) * 0.25).half()
    return dy, w, res


def _check_rounding(got, dy, w, res, Hi, Wi, k, stride, mult, *, mfma, what):
    ref = U.dgrad_ref(dy, w, res, Hi, Wi, k, stride, mult)
    A = U.dgrad_abs_ref(dy, w, Hi, Wi, k, stride, mult)
    r = torch.zeros_like(ref) if res is None else res.double().abs()
    bound = (2.0 if mfma else 1.0) * 2.0 ** -11 * ref.abs() + 2.0 ** -25 + 2.0 * k * k * mult * 2.0 ** -24 * (A + r)
    frac = ((got.double() - ref).abs() / bound)
    worst = float(frac.max())
    print(f"[dw-bwd rounding] {what}: worst |got - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: {worst:.3f} of the derived bound at {tuple(int(v) for v in (frac == frac.max()).nonzero()[0])}"
    return worst


# ================================================================================================ input gradient, VALU
@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("k,stride,mult,Ci,Hi,Wi", U.DGRAD_CASES)
def test_dgrad_valu_exact(k, stride, mult, Ci, Hi, Wi, with_res):
    B = 2
    assert U.dgrad_route(B, Hi, Wi, Ci, k, stride, mult) == f"dw_dgrad_kernel<{k},{stride},{mult}>"
    assert U.dgrad_bound(k, mult, bool(with_res)) < 2048
    _, dy, w, res = _exact_inputs(B, Ci, Hi, Wi, k, stride, mult)
    res = res if with_res else None
    got, nsat = _dgrad(dy, w.float(), res, Hi, Wi, k, stride, mult)
    assert torch.equal(got.to(torch.int64), U.dgrad_int(dy, w, res, Hi, Wi, k, stride, mult)) and nsat == 0


@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("k,stride,mult,Ci,Hi,Wi", U.DGRAD_CASES)
def test_dgrad_valu_rounding(k, stride, mult, Ci, Hi, Wi, with_res):
    B = 2
    dy, w, res = _gauss_inputs(B, Ci, Hi, Wi, k, stride, mult)
    res = res if with_res else None
    got, nsat = _dgrad(dy, w, res, Hi, Wi, k, stride, mult)
    assert nsat == 0
    _check_rounding(got, dy, w, res, Hi, Wi, k, stride, mult, mfma=False, what=f"VALU <{k},{stride},{mult}> Ci={Ci} {Hi}x{Wi} res={with_res}")


@pytest.mark.parametrize("k,stride,mult", U.INSTANCES)
def test_dgrad_round_w(k, stride, mult):
    """taps 1 + 2^-10 (not bf16 values), dy = 1024 at one position: round_w = 1 differentiates the forward that read bf16 taps (exactly 1024), round_w = 0 the fp32 taps
    (exactly 1025)"""
    B, Ci, Hi, Wi = 2, 8, 9, 14
    Co, Ho, Wo = Ci * mult, U.out_size(Hi, k, stride), U.out_size(Wi, k, stride)
    dy = torch.zeros(B, Co, Ho, Wo)
    dy[1, 3, Ho // 2, Wo // 2] = 1024.0
    w = torch.full((k * k, Co), 1.0 + 2.0 ** -10)
    stamp = U.dgrad_int(dy.to(torch.int64) // 1024, torch.ones(k * k, Co, dtype=torch.int64), None, Hi, Wi, k, stride, mult)   # 1 where the element reaches
    assert int(stamp.sum()) > 1
    for round_w, val in ((1, 1024), (0, 1025)):
        got, nsat = _dgrad(dy, w, None, Hi, Wi, k, stride, mult, round_w=round_w)
        assert torch.equal(got.to(torch.int64), stamp * val) and nsat == 0, round_w


# ================================================================================================ input gradient, MFMA
@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("k,C,H,W", U.DGRAD_MFMA_CASES)
def test_dgrad_mfma_exact(k, C, H, W, with_res):
    B = 2
    assert U.dgrad_mfma_route(B, H, W, C, k) == f"dwconv_march_kernel<{k},GRAD>"
    _, dy, w, res = _exact_inputs(B, C, H, W, k, 1, 1)
    res = res if with_res else None
    ref = U.dgrad_int(dy, w, res, H, W, k, 1, 1)
    got, nsat = _dgrad(dy, w.float(), res, H, W, k, 1, 1, mfma=True)
    assert torch.equal(got.to(torch.int64), ref) and nsat == 0
    valu, nsat_v = _dgrad(dy, w.float(), res, H, W, k, 1, 1)      # the same inputs on the VALU kernel: the same bits
    assert torch.equal(_bits(valu), _bits(got)) and nsat_v == 0


def test_dgrad_mfma_needs_the_flipped_table():
    """the table of the UNflipped taps gives another answer on asymmetric taps: the exact test above would notice a forgotten flip"""
    k, C, H, W = 3, 32, 16, 20
    _, dy, w, _ = _exact_inputs(2, C, H, W, k, 1, 1)
    got, _ = _dgrad(dy, w.float(), None, H, W, k, 1, 1, mfma=True, flip=False)
    assert not torch.equal(got.to(torch.int64), U.dgrad_int(dy, w, None, H, W, k, 1, 1))
    assert torch.equal(got.to(torch.int64), U.dgrad_int(dy, torch.flip(w, dims=[0]), None, H, W, k, 1, 1))


@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("k,C,H,W", U.DGRAD_MFMA_CASES)
def test_dgrad_mfma_rounding(k, C, H, W, with_res):
    B = 2
    dy, w, res = _gauss_inputs(B, C, H, W, k, 1, 1)
    w = w.half().float()                       # the table holds fp16 taps: the reference reads the same stored values
    res = res if with_res else None
    got, nsat = _dgrad(dy, w, res, H, W, k, 1, 1, mfma=True)
    assert nsat == 0
    _check_rounding(got, dy, w, res, H, W, k, 1, 1, mfma=True, what=f"MFMA k={k} C={C} {H}x{W} res={with_res}")


@pytest.mark.parametrize("k,C,H,W", U.DGRAD_MFMA_REFUSED)
def test_dgrad_mfma_refusals_enqueue_nothing(k, C, H, W):
    B = 2
    assert U.dgrad_mfma_route(B, H, W, C, k) is None
    n = B * H * W * max(C, 32)
    dy = torch.ones(n, dtype=torch.float16, device=DEV)
    tab = torch.ones(4 * 7 * 4 * 256, dtype=torch.float16, device=DEV)
    dx = torch.full((n,), NAN, dtype=torch.float16, device=DEV)
    sat = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib().fv_op_dw_dgrad_mfma(dy.data_ptr(), tab.data_ptr(), None, dx.data_ptr(), B, H, W, C, k, sat.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc in (FV_ERR_ARG, FV_ERR_UNSUPPORTED) and rc != 0
    assert bool(torch.isnan(dx).all()) and int(sat[0]) == 0


def test_dgrad_argument_checks_enqueue_nothing():
    B, Ci, Hi, Wi = 2, 8, 9, 14
    dy = torch.ones(B * Hi * Wi * Ci * 2, dtype=torch.float16, device=DEV)
    w = torch.ones(49 * 16, dtype=torch.float32, device=DEV)
    dx = torch.full((B * Hi * Wi * Ci,), NAN, dtype=torch.float16, device=DEV)
    f = lib().fv_op_dw_dgrad
    bad = [f(None, w.data_ptr(), None, dx.data_ptr(), B, Hi, Wi, Ci, 3, 1, 1, 0, None, stream()),
           f(dy.data_ptr(), w.data_ptr(), None, dx.data_ptr(), B, Hi, Wi, 12, 3, 1, 1, 0, None, stream()),       # Ci % 8
           f(dy.data_ptr(), w.data_ptr(), None, dx.data_ptr(), B, Hi, Wi, Ci, 5, 1, 1, 0, None, stream()),       # no such instance
           f(dy.data_ptr(), w.data_ptr(), None, dx.data_ptr(), B, Hi, Wi, Ci, 7, 2, 1, 0, None, stream()),
           f(dy.data_ptr(), w.data_ptr(), None, dx.data_ptr(), 0, Hi, Wi, Ci, 3, 1, 1, 0, None, stream()),
           f(dy.data_ptr(), w.data_ptr(), None, dx.data_ptr() + 2, B, Hi, Wi, Ci, 3, 1, 1, 0, None, stream()),   # misaligned
           f(dy.data_ptr(), w.data_ptr(), None, dx.data_ptr(), B, Hi, Wi, Ci, 3, 1, 1, 2, None, stream())]       # round_w
    torch.cuda.synchronize()
    assert all(rc in (FV_ERR_ARG, FV_ERR_UNSUPPORTED) for rc in bad), bad
    assert bool(torch.isnan(dx).all())


# ================================================================================================ selection
def _positions(Ho, Wo):
    """four corners (the last one is the last valid output position) and an interior element"""
    return [(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1), (Ho // 2, Wo // 2 - 1)]


def _stamp(B, Ci, Hi, Wi, k, stride, mult, w, placed):
    """the flipped kernel stamped at each placed element (b, co, yo, xo, v), clipped at the border -- written with explicit indices, independently of dgrad_int"""
    pad = k // 2
    dx = torch.zeros(B, Ci, Hi, Wi, dtype=torch.int64)
    for (b, co, yo, xo, v) in placed:
        for ky in range(k):
            for kx in range(k):
                yi, xi = yo * stride - pad + ky, xo * stride - pad + kx
                if 0 <= yi < Hi and 0 <= xi < Wi:
                    dx[b, co // mult, yi, xi] += int(w[ky * k + kx, co]) * v
    return dx


def _selection_case(B, Ci, Hi, Wi, k, stride, mult, chans):
    Co, Ho, Wo = Ci * mult, U.out_size(Hi, k, stride), U.out_size(Wi, k, stride)
    dy = torch.zeros(B, Co, Ho, Wo, dtype=torch.int64)
    placed = []
    for i, ((yo, xo), ci) in enumerate(zip(_positions(Ho, Wo), chans)):
        b, co, v = i % B, ci * mult + (i % mult), (1 if i % 2 == 0 else -1)
        dy[b, co, yo, xo] = v
        placed.append((b, co, yo, xo, v))
    t = torch.arange(k * k).view(k * k, 1)
    w = (t + 1) + 50 * (torch.arange(Co).view(1, Co) % 4)          # every tap of a channel distinct: 1 .. 199
    return dy, w, placed


@pytest.mark.parametrize("k,stride,mult,Hi,Wi", [(k, s, m, Hi, Wi) for (k, s, m) in U.INSTANCES for (Hi, Wi) in ([(9, 14), (10, 13)] if s == 2 else [(11, 17)])])
def test_dgrad_valu_selection(k, stride, mult, Hi, Wi):
    B, Ci = 2, 24
    dy, w, placed = _selection_case(B, Ci, Hi, Wi, k, stride, mult, [0, 7, 8, 15, 23])
    want = _stamp(B, Ci, Hi, Wi, k, stride, mult, w, placed)
    assert torch.equal(want, U.dgrad_int(dy, w, None, Hi, Wi, k, stride, mult))
    got, _ = _dgrad(dy, w.float(), None, Hi, Wi, k, stride, mult)
    assert torch.equal(got.to(torch.int64), want)


@pytest.mark.parametrize("k,C,H,W", [(7, 32, 19, 33), (3, 32, 16, 20), (7, 64, 16, 16)])
def test_dgrad_mfma_selection(k, C, H, W):
    B = 2
    dy, w, placed = _selection_case(B, C, H, W, k, 1, 1, [0, 7, 8, 31, 16])
    want = _stamp(B, C, H, W, k, 1, 1, w, placed)
    got, _ = _dgrad(dy, w.float(), None, H, W, k, 1, 1, mfma=True)
    assert torch.equal(got.to(torch.int64), want)


@pytest.mark.parametrize("route,k,stride,mult,Ci,Hi,Wi,B", U.WGRAD_CASES)
def test_wgrad_selection(route, k, stride, mult, Ci, Hi, Wi, B):
    """one dy element per chosen channel: dw[t][co] is the x value under tap t of that output position -- exactly 0 where the tap falls outside the map -- and every
    channel without a dy element gets exact zeros"""
    Co, Ho, Wo, pad = Ci * mult, U.out_size(Hi, k, stride), U.out_size(Wi, k, stride), k // 2
    g = _gen(k, stride, mult, Ci, Hi, Wi, 5)
    x = _ints((B, Ci, Hi, Wi), -100, 100, g)
    x[x == 0] = 7                                            # no zero inside the map: a tap outside it is the only way to a 0
    dy = torch.zeros(B, Co, Ho, Wo, dtype=torch.int64)
    want_w, want_b = torch.zeros(k * k, Co, dtype=torch.int64), torch.zeros(Co, dtype=torch.int64)
    chans = [0, Co // 2 - 1, Co // 2, Co - 1, 3]
    for i, ((yo, xo), co) in enumerate(zip(_positions(Ho, Wo), chans)):
        b, v = i % B, (1 if i % 2 == 0 else -1)
        dy[b, co, yo, xo] = v
        want_b[co] = v
        for ky in range(k):
            for kx in range(k):
                yi, xi = yo * stride - pad + ky, xo * stride - pad + kx
                if 0 <= yi < Hi and 0 <= xi < Wi:
                    want_w[ky * k + kx, co] = v * int(x[b, co // mult, yi, xi])
    assert len(set(chans)) == 5
    dw, db = _wgrad(x, dy, k, stride, mult, route)
    assert torch.equal(dw.double(), want_w.double()) and torch.equal(db.double(), want_b.double())


# ================================================================================================ tap + bias gradients
@pytest.mark.parametrize("route,k,stride,mult,Ci,Hi,Wi,B", U.WGRAD_CASES)
def test_wgrad_exact(route, k, stride, mult, Ci, Hi, Wi, B):
    Ho, Wo = U.out_size(Hi, k, stride), U.out_size(Wi, k, stride)
    assert U.wgrad_bound(B, Ho, Wo) < 2 ** 24
    x, dy, _, _ = _exact_inputs(B, Ci, Hi, Wi, k, stride, mult)
    dw, db = _wgrad(x, dy, k, stride, mult, route)
    rw, rb = U.wgrad_int(x, dy, k, stride, mult)
    assert torch.equal(dw.double(), rw.double()) and torch.equal(db.double(), rb.double())


@pytest.mark.parametrize("route,k,stride,mult,Ci,Hi,Wi,B", U.WGRAD_CASES)
def test_wgrad_gaussian(route, k, stride, mult, Ci, Hi, Wi, B):
    """the tolerance the project already uses for this op (test_dw_wgrad_matches_autograd), now on every route and instance"""
    g = _gen(k, stride, mult, Ci, Hi, Wi, 9)
    Co, Ho, Wo = Ci * mult, U.out_size(Hi, k, stride), U.out_size(Wi, k, stride)
    x = torch.randn(B, Ci, Hi, Wi, generator=g).bfloat16().float()
    dy = (torch.randn(B, Co, Ho, Wo, generator=g) * 0.25).half()
    dw, db = _wgrad(x, dy, k, stride, mult, route)
    rw, rb = U.wgrad_ref(x, dy, k, stride, mult)
    check_close(dw, rw.float(), rel=2e-5, amax=1e-4, what=f"{route} tap gradients Ci={Ci} {Hi}x{Wi} B={B}")
    check_close(db, rb.float(), rel=2e-5, amax=1e-4, what=f"{route} bias gradient Ci={Ci} {Hi}x{Wi} B={B}")


# ================================================================================================ saturation
def _sat_case(B, Ci, Hi, Wi, k, stride, mult, big, res_val):
    """centre tap 2, others 0: conv^T(dy)[yo s][xo s][ci] = 2 sum_q dy[yo][xo][ci mult + q].  `big` goes to chosen elements over a small-integer background:
    two channels of ONE 8-channel group of a pixel (one cell), two groups of another pixel (two cells), a negative one, the last pixel of the map"""
    Co, Ho, Wo = Ci * mult, U.out_size(Hi, k, stride), U.out_size(Wi, k, stride)
    g = _gen(k, stride, mult, Ci, Hi, Wi, 11)
    dy = _ints((B, Co, Ho, Wo), -4, 4, g)
    w = torch.zeros(k * k, Co, dtype=torch.int64)
    w[k * k // 2] = 2
    spots = [(0, 0, 1, 2, 1), (0, 5, 1, 2, 1), (1, 1, Ho - 1, Wo - 1, 1), (1, Ci - 1, Ho - 1, Wo - 1, -1), (0, 3, 0, 0, -1), (1, 2, Ho // 2, 3, 1)]
    if Ci == 8:
        spots[3] = (1, Ci - 1, Ho - 2, Wo - 1, -1)           # one group per pixel: keep the negative one in a cell of its own
    res = _ints((B, Ci, Hi, Wi), -512, 512, g)
    for (b, ci, yo, xo, sign) in spots:
        dy[b, ci * mult:(ci + 1) * mult, yo, xo] = 0
        dy[b, ci * mult, yo, xo] = sign * big
        if res_val is not None:
            res[b, ci, yo * stride, xo * stride] = sign * res_val
    return dy, w, (res if res_val is not None else None)


def _sat_expect(dy, w, res, Hi, Wi, k, stride, mult, mfma):
    """(dx, cells): the VALU kernel clamps res + conv summed in fp32; the MFMA kernel sees an out-of-range conv value as out of range whatever res holds"""
    conv = U.dgrad_int(dy, w, None, Hi, Wi, k, stride, mult).double()
    if mfma:
        conv = torch.where(conv.abs() > U.F16_MAX, torch.sign(conv) * float("inf"), conv)
    total = conv if res is None else conv + res.double()
    over = total.abs() > U.F16_MAX
    B, Ci = total.shape[0], total.shape[1]
    cells = int(over.view(B, Ci // 8, 8, Hi, Wi).any(2).sum())
    return total.clamp(-U.F16_MAX, U.F16_MAX), cells


SAT_ROUTES = [("valu", k, s, m, 16 if (k, s, m) != (3, 1, 1) else 8, Hi, Wi) for (k, s, m), (Hi, Wi) in zip(U.INSTANCES, [(11, 17), (11, 17), (9, 14), (10, 13), (11, 17)])] + \
             [("mfma", 7, 1, 1, 32, 19, 33), ("mfma", 3, 1, 1, 64, 16, 20)]


@pytest.mark.parametrize("kind,big,res_val,cells_valu,cells_mfma", [
    ("clamps, no residual", 60000, None, 5, 5),
    ("nothing clamps", 30000, None, 0, 0),                     # 2 x 30000 = 60000 is an fp16 value: exact, counter stays 0
    ("nothing clamps, residual", 30000, 5000, 0, 0),           # 65000 rounds to an fp16 value below 65504: no clamp
    ("residual pushes a finite sum over", 30000, 6000, 5, 5),  # 60000 + 6000: both routes clamp the SUM and count
    ("residual pulls a clamped conv back", 60000, -60000, 0, 5)])   # VALU: 120000 - 60000 = 60000, no clamp.  MFMA: conv itself out of range -> +-65504, counted
@pytest.mark.parametrize("route,k,stride,mult,Ci,Hi,Wi", SAT_ROUTES)
def test_dgrad_saturation_is_clamped_and_counted(route, k, stride, mult, Ci, Hi, Wi, kind, big, res_val, cells_valu, cells_mfma):
    B, mfma = 2, route == "mfma"
    if mfma:
        assert U.dgrad_mfma_route(B, Hi, Wi, Ci, k) is not None
    dy, w, res = _sat_case(B, Ci, Hi, Wi, k, stride, mult, big, res_val)
    want, cells = _sat_expect(dy, w, res, Hi, Wi, k, stride, mult, mfma)
    # the six spots are five cells (two share a group) -- or four where Ci = 8 ... computed, then pinned to the table above
    assert cells == (cells_mfma if mfma else cells_valu), (kind, cells)
    got, nsat = _dgrad(dy, w.float(), res, Hi, Wi, k, stride, mult, mfma=mfma)
    assert bool(torch.isfinite(got).all())
    want16 = want.to(torch.float16)                            # in-range sums beyond the exact-integer range (65000) round to fp16 once, as the kernels do
    assert torch.equal(_bits(got), _bits(want16)), kind
    assert nsat == cells, (kind, nsat, cells)
    if cells:
        assert int((got.double().abs() == U.F16_MAX).sum()) >= cells
    # a null counter is allowed and changes nothing else
    got0, nsat0 = _dgrad(dy, w.float(), res, Hi, Wi, k, stride, mult, mfma=mfma, with_sat=False)
    assert torch.equal(_bits(got0), _bits(got)) and nsat0 == 0
