"""-m gpu: every kernel instance of the depthwise convs' forward, each on its own entry point, against exact or float64 references (tests/dw_fwd_util.py).

  fv_op_dwconv          dwconv_tile_kernel<3 | 7> (stride 1, mult 1, W >= 32, C % 32 == 0) and dwconv_kernel<k, stride, mult>, the five instances
  fv_op_dwconv_mfma     dwconv_march_kernel<7> (H >= 16), dwconv_mfma_kernel<7,8> (H < 16), dwconv_mfma_kernel<3,8>
  fv_op_dwconv_s2_mfma  dwconv_s2_mfma_kernel, persistent: one case where blocks walk three tiles, across an image boundary, with a short last XCD range
  fv_op_dwconv_pair     dwpair_march_kernel<64,16> and <32,32>, cut into row segments and uncut over four units

Every case asserts the route it was written for against the route mirror (dw_fwd_util.*_route), the stride-2 one with the device's own CU count; the CPU file
tests/test_dw_forward_reference_host.py checks that the tables cover every reachable instance and that the checks below fail on planted defects.

Every launch here writes into a NaN-filled output that sits inside a larger allocation with a sentinel pattern before and behind it, runs twice into fresh
buffers, and must leave the sentinels and the bits of its inputs, tables and biases alone, write every element, and give the same bits both times.

EXACT: integer inputs whose every intermediate and output is an integer of magnitude <= 256 (a bf16 value, exact in fp32 in any order): the output equals the
int64 reference element for element.  For the pair this pins that x' outside the map is the 7x7's zero padding (b3 is non-zero) and that t is computed from x'.
SELECTION: a single 1 per image position, in every channel, taps 1 + (ky k + kx) + (c % 5), bias 0: the output is the mirrored tap patch clipped to the map and
+0 elsewhere, bit for bit -- at the corners, both sides of every strip-column boundary, of the first unit and group row boundaries, of every row-group boundary of
the pair (its segment starts among them), at even and odd coordinates.  Different positions go to different batch entries (or lie 2k apart).
GAUSSIAN, per element against float64 on the stored values, A = sum |w x| + |b|, delta = 2 k^2 2^-24 A:
  |got - ref| <= hulp(|ref| + D) + D,  D = delta, or with GELU  D = E + 1.13 delta  (E: dw_fwd_util.GELU_ERR, the error csrc/common.h documents)
hulp = bf16's half-ulp AT the value, 2^(floor(log2 v) - 8): what round-to-nearest can use up and truncation exceeds by up to 2.  (With 2^-9 v in its place -- the
half-ulp relative to the top of a binade only -- a correctly rounded result is itself over by up to 1.98: each case prints that figure next to the asserted one.)
The pair's t is held against conv7 of the x' the kernel returned.  Bounds are derived, not measured; docs/kernels.md records the MI355X fractions.
FOOTPRINT: image b's result has the same bits alone and between two images of +-1e4, and equals the integer reference.
REFUSALS enqueue nothing: non-zero return code, the pre-filled output keeps its pattern."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import dw_fwd_util as U  # noqa: E402
from gpu_util import DEV, call, lib, stream  # noqa: E402

NAN = float("nan")
SENT, GUARD = 0x5A5A, 4096          # sentinel pattern and elements of it before and behind every output


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device (no CPU fallback in the product path)")


_DEVICE_ERROR = []


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a launch that ended in a device error (not a wrong value) leaves the device in an unknown state: nothing more is launched on it from this file"""
    if _DEVICE_ERROR:
        pytest.exit(f"a device error earlier in this file: {_DEVICE_ERROR[0]}", returncode=3)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ launching
def _out(n):
    """(whole int16 allocation, the NaN-filled bf16 output of n elements inside it)"""
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int16, device=DEV)
    y = buf[GUARD:GUARD + n].view(torch.bfloat16)
    y.fill_(NAN)
    return buf, y


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())


def _raw(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _twice(launch, ins, sizes, what):
    """launch(outs) enqueues the op on `outs` (bf16 device views).  Runs it twice into fresh guarded buffers; returns the first run's outputs on the CPU (flat bf16)"""
    before = [_raw(t).clone() for t in ins]
    runs = []
    for rep in range(2):
        bufs = [_out(n) for n in sizes]
        call(launch([y for (_, y) in bufs]), what)
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            _DEVICE_ERROR.append(f"{what}: {e}")
            raise
        assert all(_guards_intact(b, n) for (b, _), n in zip(bufs, sizes)), f"{what}: written before or behind the output"
        runs.append([y.cpu() for (_, y) in bufs])
    assert all(torch.equal(_raw(t), s) for t, s in zip(ins, before)), f"{what}: an input, table or bias changed"
    assert all(torch.equal(_raw(a), _raw(b)) for a, b in zip(runs[0], runs[1])), f"{what}: two launches differ"
    assert not any(bool(torch.isnan(y.float()).any()) for y in runs[0]), f"{what}: an output element was not written (or is NaN)"
    return runs[0]


def _conv(entry, x, w, b, k, stride, mult, gelu=0):
    """x (B,Ci,H,W), w (Co,1,k,k), b (Co) CPU tensors of values the kernel can hold -> y (B,Co,Ho,Wo) fp32 on the CPU.  entry: "valu" | "mfma" | "s2"."""
    B, Ci, H, W = x.shape
    Co, Ho, Wo = Ci * mult, U.out_size(H, k, stride), U.out_size(W, k, stride)
    xd = U.nhwc(x.to(torch.float32)).to(torch.bfloat16).to(DEV)
    bd = b.to(torch.float32).to(DEV).contiguous()
    if entry == "valu":
        wd = U.tap_major(w.to(torch.float32), k).to(DEV)
        launch = lambda o: lib().fv_op_dwconv(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), o[0].data_ptr(), B, H, W, Ci, k, stride, mult, gelu, stream())  # noqa: E731
    elif entry == "mfma":
        wd = U.toeplitz(w.to(torch.float32), k).to(torch.bfloat16).to(DEV).contiguous()
        launch = lambda o: lib().fv_op_dwconv_mfma(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), o[0].data_ptr(), B, H, W, Ci, k, gelu, stream())  # noqa: E731
    else:
        assert (k, stride, mult) == (7, 2, 2)
        wd = U.toeplitz_s2(w.to(torch.float32)).to(torch.bfloat16).to(DEV).contiguous()
        launch = lambda o: lib().fv_op_dwconv_s2_mfma(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), o[0].data_ptr(), B, H, W, Ci, gelu, stream())  # noqa: E731
    (y,) = _twice(launch, [xd, wd, bd], [B * Ho * Wo * Co], f"fv_op_dwconv[{entry}] k{k} s{stride} m{mult} C{Ci} {H}x{W} B{B}")
    return U.nchw(y.float().view(B, Ho, Wo, Co))


def _pair(x, w3, b3, w7, b7):
    """-> (x', t) (B,C,H,W) fp32 on the CPU"""
    B, C, H, W = x.shape
    xd = U.nhwc(x.to(torch.float32)).to(torch.bfloat16).to(DEV)
    t3 = U.toeplitz(w3.to(torch.float32), 3).to(torch.bfloat16).to(DEV).contiguous()
    t7 = U.toeplitz(w7.to(torch.float32), 7).to(torch.bfloat16).to(DEV).contiguous()
    b3d, b7d = b3.to(torch.float32).to(DEV).contiguous(), b7.to(torch.float32).to(DEV).contiguous()
    launch = lambda o: lib().fv_op_dwconv_pair(xd.data_ptr(), t3.data_ptr(), b3d.data_ptr(), t7.data_ptr(), b7d.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), B, H, W, C, stream())  # noqa: E731
    y1, y2 = _twice(launch, [xd, t3, b3d, t7, b7d], [B * H * W * C] * 2, f"fv_op_dwconv_pair C{C} {H}x{W} B{B}")
    return U.nchw(y1.float().view(B, H, W, C)), U.nchw(y2.float().view(B, H, W, C))


# every single-conv case of the tables as (entry, kernel, k, stride, mult, Ci, H, W, B)
def _route(entry, B, H, W, C, k, stride, mult):
    if entry == "valu":
        return U.dwconv_route(B, H, W, C, k, stride, mult)
    if entry == "mfma":
        return U.dwconv_mfma_route(B, H, W, C, k)
    return U.dwconv_s2_route(B, H, W, C, _cus())


CONV_CASES = ([("valu", f"dwconv_kernel<{k},{s},{m}>", k, s, m, Ci, H, W, 2) for (k, s, m, Ci, H, W) in U.VALU_CASES]
              + [("valu", f"dwconv_tile_kernel<{k}>", k, 1, 1, C, H, W, 2) for (k, C, H, W) in U.TILE_CASES]
              + [("mfma", kern, k, 1, 1, C, H, W, 2) for (kern, k, C, H, W) in U.MFMA_CASES]
              + [("s2", "dwconv_s2_mfma_kernel", 7, 2, 2, C, H, W, B) for (C, H, W, B) in U.S2_CASES])
_ids = [f"{c[1]}-C{c[5]}-{c[6]}x{c[7]}-B{c[8]}" for c in CONV_CASES]


def _assert_route(entry, kern, k, stride, mult, C, H, W, B):
    r = _route(entry, B, H, W, C, k, stride, mult)
    assert r is not None and r["kernel"] == kern, (r, kern)
    if (C, H, W, B) == U.S2_WALK_CASE and entry == "s2":
        # the three conditions of the walking case, through the mirror and for THIS device's CU count -- not trusted from the shape
        p = U.dwconv_s2_walk_properties(B, H, W, C, _cus())
        assert r["tpx"] > r["chains"] and p["longest"] >= 3, (r, p)
        assert p["crosses_images"] and p["last_xcd_short"] and r["tiles"] % 8 != 0 and p["complete"], (r, p)
        assert B * H * W * C * 2 < 64 * 2 ** 20
    return r


# ================================================================================================ exact
@pytest.mark.parametrize("entry,kern,k,stride,mult,C,H,W,B", CONV_CASES, ids=_ids)
def test_conv_exact(entry, kern, k, stride, mult, C, H, W, B):
    _assert_route(entry, kern, k, stride, mult, C, H, W, B)
    assert U.exact_budget(k) <= U.EXACT_LIMIT
    x, w, b = U.exact_inputs(B, C, H, W, k, stride, mult)
    U.check_exact(_conv(entry, x, w, b, k, stride, mult), U.conv_int(x, w, b, k, stride, mult), f"{kern} C{C} {H}x{W}")


@pytest.mark.parametrize("kern,C,H,W,B,nseg", U.PAIR_CASES)
def test_pair_exact(kern, C, H, W, B, nseg):
    r = U.dwconv_pair_route(B, H, W, C)
    assert r["kernel"] == kern and r["nseg"] == nseg and (nseg > 1 or r["nstrips"] >= 256 or r["groups"] < 4), r
    if r["nstrips"] >= 256:
        assert r["nseg"] == 1 and r["groups"] >= 4                     # the uncut march over at least four units
    assert max(U.exact_budget_pair()) <= U.EXACT_LIMIT
    x, w3, b3, w7, b7 = U.exact_inputs_pair(B, C, H, W)
    xp_ref = U.conv_int(x, w3, b3, 3, 1, 1)
    xp, t = _pair(x, w3, b3, w7, b7)
    U.check_exact(xp, xp_ref, f"{kern} x' C{C} {H}x{W} B{B}")
    U.check_exact(t, U.conv_int(xp_ref, w7, b7, 7, 1, 1), f"{kern} t C{C} {H}x{W} B{B}")


# ================================================================================================ Gaussian
@functools.lru_cache(maxsize=2)
def _gauss_case(entry, k, stride, mult, C, H, W, B):
    x, w, b = U.gauss_inputs(B, C, H, W, k, stride, mult, table=(entry != "valu"))
    return x, w, b, U.conv_f64(x, w, b, k, stride, mult), U.conv_abs(x, w, b, k, stride, mult)


def _report(got, pre, A, k, gelu, what):
    lit = U.gauss_fraction(got, pre, A, k, gelu, literal=True)[0]
    print(f"[dw-fwd gauss] {what}: with 2^-9 |ref| as the rounding term = {lit:.3f}")
    return U.check_gauss(got, pre, A, k, gelu, what)


@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("entry,kern,k,stride,mult,C,H,W,B", CONV_CASES, ids=_ids)
def test_conv_gaussian(entry, kern, k, stride, mult, C, H, W, B, gelu):
    _assert_route(entry, kern, k, stride, mult, C, H, W, B)
    x, w, b, pre, A = _gauss_case(entry, k, stride, mult, C, H, W, B)
    got = _conv(entry, x, w, b, k, stride, mult, gelu)
    _report(got, pre, A, k, U.gelu_of(kern) if gelu else None, f"{kern} gelu={gelu} C{C} {H}x{W} B{B}")


@pytest.mark.parametrize("kern,C,H,W,B,nseg", U.PAIR_CASES)
def test_pair_gaussian(kern, C, H, W, B, nseg):
    assert U.dwconv_pair_route(B, H, W, C)["kernel"] == kern and U.gelu_of(kern) is None
    x, w3, b3 = U.gauss_inputs(B, C, H, W, 3, 1, 1, 5, table=True)
    _, w7, b7 = U.gauss_inputs(B, C, H, W, 7, 1, 1, 6, table=True)
    xp, t = _pair(x, w3, b3, w7, b7)
    _report(xp, U.conv_f64(x, w3, b3, 3, 1, 1), U.conv_abs(x, w3, b3, 3, 1, 1), 3, None, f"{kern} x' C{C} {H}x{W} B{B}")
    # t against the 7x7 of the x' the kernel RETURNED (float64 on its bits): a 7x7 fed anything else -- the un-rounded x' -- is off by more than its own rounding
    _report(t, U.conv_f64(xp, w7, b7, 7, 1, 1), U.conv_abs(xp, w7, b7, 7, 1, 1), 7, None, f"{kern} t C{C} {H}x{W} B{B}")


# ================================================================================================ selection
def _rows_cols(kern, H, W, stride):
    """the rows and columns (input coordinates) on both sides of the kernel's strip, tile, unit and group boundaries"""
    if kern.startswith("dwconv_kernel"):
        return [], U.boundary_pairs(4 * stride, W, limit=1)                                        # a thread's four outputs
    if kern.startswith("dwconv_s2_mfma"):
        return U.boundary_pairs(16, H, limit=2), U.boundary_pairs(32, W)                           # 8 x 16 output tiles
    if kern.startswith("dwconv_march"):
        return U.boundary_pairs(8, H, limit=2) + U.boundary_pairs(8, H, first=-5, limit=2), U.boundary_pairs(32, W)      # groups 8g, units 8u + 3
    if kern.startswith("dwpair"):
        tw = 16 if "<64,16>" in kern else 32
        # every group boundary 8g (the segment starts 8 g0 are among them whatever nseg the batch gives), x' units 8u + 3, x units 8u + 4
        return U.boundary_pairs(8, H) + U.boundary_pairs(8, H, first=-5, limit=2) + U.boundary_pairs(8, H, first=-4, limit=2), U.boundary_pairs(tw, W)
    return U.boundary_pairs(8, H, limit=2), U.boundary_pairs(32, W)                                # 8 x 32 tiles


SELECTION_CASES = ([("valu", f"dwconv_kernel<{k},{s},{m}>", k, s, m, 24, H, W) for (k, s, m) in U.INSTANCES for (H, W) in U.VALU_MAPS[s]]
                   + [("valu", f"dwconv_tile_kernel<{k}>", k, 1, 1, C, H, W) for k in (3, 7) for (C, H, W) in [(64, 19, 33), (96, 9, 70)]]
                   + [("mfma", "dwconv_mfma_kernel<7,8>", 7, 1, 1, 64, 15, 37), ("mfma", "dwconv_mfma_kernel<7,8>", 7, 1, 1, 32, 9, 16),
                      ("mfma", "dwconv_mfma_kernel<3,8>", 3, 1, 1, 64, 33, 47), ("mfma", "dwconv_mfma_kernel<3,8>", 3, 1, 1, 32, 16, 20),
                      ("mfma", "dwconv_march_kernel<7>", 7, 1, 1, 64, 19, 33), ("mfma", "dwconv_march_kernel<7>", 7, 1, 1, 32, 24, 70),
                      ("s2", "dwconv_s2_mfma_kernel", 7, 2, 2, 64, 18, 34), ("s2", "dwconv_s2_mfma_kernel", 7, 2, 2, 96, 40, 64)])


@pytest.mark.parametrize("entry,kern,k,stride,mult,C,H,W", SELECTION_CASES, ids=[f"{c[1]}-C{c[5]}-{c[6]}x{c[7]}" for c in SELECTION_CASES])
def test_conv_selection(entry, kern, k, stride, mult, C, H, W):
    rows, cols = _rows_cols(kern, H, W, stride)
    pos = U.selection_positions(H, W, rows, cols)
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= set(pos)
    if stride == 2:
        assert {(r % 2, c % 2) for (r, c) in pos} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    images = U.pack_positions(pos, k)
    B = len(images)
    assert _route(entry, B, H, W, C, k, stride, mult)["kernel"] == kern
    x, w = U.selection_input(images, C, H, W), U.selection_taps(C * mult, k)
    want = U.selection_expected(images, w, H, W, k, stride, mult)                                  # both outputs of a channel under mult 2: every co is compared
    got = _conv(entry, x, w, torch.zeros(C * mult), k, stride, mult)
    U.check_bits(got, want, f"{kern} C{C} {H}x{W}, {len(pos)} impulses in {B} images")


@pytest.mark.parametrize("kern,C,H,W,cut", [("dwpair_march_kernel<64,16>", 64, 50, 37, True), ("dwpair_march_kernel<64,16>", 64, 19, 37, False),
                                            ("dwpair_march_kernel<32,32>", 96, 40, 64, True), ("dwpair_march_kernel<32,32>", 32, 16, 32, False)])
def test_pair_selection(kern, C, H, W, cut):
    """(a) the 3x3 carries the selection taps and the 7x7 is the identity: x' is the 3x3's patch and t = x'.  (b) the 3x3 is the identity and the 7x7 carries the
    taps: x' = x and t is the 7x7's patch.  (Both at once would leave t sums of up to 9 x 13 x 53: no bf16 values.)"""
    rows, cols = _rows_cols(kern, H, W, 1)
    pos = U.selection_positions(H, W, rows, cols)
    images = U.pack_positions(pos, 7)
    B = len(images)
    r = U.dwconv_pair_route(B, H, W, C)
    assert r["kernel"] == kern and (r["nseg"] > 1) == cut, r
    for g0 in r["starts"][1:]:
        assert {8 * g0 - 1, 8 * g0} <= {p[0] for p in pos}                                         # both sides of every segment boundary carry impulses
    x, zero = U.selection_input(images, C, H, W), torch.zeros(C)
    s3, s7 = U.selection_taps(C, 3), U.selection_taps(C, 7)
    xp, t = _pair(x, s3, zero, U.identity_taps(C, 7), zero)
    want = U.selection_expected(images, s3, H, W, 3, 1, 1)
    U.check_bits(xp, want, f"{kern} x' = the 3x3's patch")
    U.check_bits(t, want, f"{kern} t = x' under an identity 7x7")
    xp, t = _pair(x, U.identity_taps(C, 3), zero, s7, zero)
    U.check_bits(xp, x, f"{kern} x' = x under an identity 3x3")
    U.check_bits(t, U.selection_expected(images, s7, H, W, 7, 1, 1), f"{kern} t = the 7x7's patch")


# ================================================================================================ footprint
def _big(shape, g):
    """finite values of magnitude 1e4 (bf16: 9984), either sign"""
    return (2 * torch.randint(0, 2, shape, generator=g) - 1).to(torch.float32) * 9984.0


FOOTPRINT_CASES = ([("valu", f"dwconv_kernel<{k},{s},{m}>", k, s, m, 24, *U.VALU_MAPS[s][0]) for (k, s, m) in U.INSTANCES]
                   + [("valu", "dwconv_tile_kernel<3>", 3, 1, 1, 64, 19, 33), ("valu", "dwconv_tile_kernel<7>", 7, 1, 1, 64, 19, 33),
                      ("mfma", "dwconv_mfma_kernel<7,8>", 7, 1, 1, 64, 15, 37), ("mfma", "dwconv_mfma_kernel<3,8>", 3, 1, 1, 96, 17, 40),
                      ("mfma", "dwconv_march_kernel<7>", 7, 1, 1, 64, 19, 33), ("s2", "dwconv_s2_mfma_kernel", 7, 2, 2, 64, 18, 34)])


@pytest.mark.parametrize("entry,kern,k,stride,mult,C,H,W", FOOTPRINT_CASES, ids=[c[1] for c in FOOTPRINT_CASES])
def test_conv_image_is_independent_of_its_neighbours(entry, kern, k, stride, mult, C, H, W):
    """the reads before and behind an image's rows: image 1 of [+-1e4, exact class, +-1e4] has the bits it has alone, and they are the integer reference"""
    assert _route(entry, 1, H, W, C, k, stride, mult)["kernel"] == kern and _route(entry, 3, H, W, C, k, stride, mult)["kernel"] == kern
    x, w, b = U.exact_inputs(1, C, H, W, k, stride, mult, 3)
    g = U.gen(C, H, W, k, 99)
    alone = _conv(entry, x, w, b, k, stride, mult)
    three = _conv(entry, torch.cat([_big(x.shape, g), x.float(), _big(x.shape, g)], 0), w, b, k, stride, mult)
    assert bool(torch.isfinite(three).all())
    assert torch.equal(U.bits16(three[1:2]), U.bits16(alone)), f"{kern}: the middle image depends on its neighbours"
    U.check_exact(alone, U.conv_int(x, w, b, k, stride, mult), kern)
    assert float(three[0].abs().max()) > 1e4 and float(three[2].abs().max()) > 1e4


@pytest.mark.parametrize("kern,C,H,W", [("dwpair_march_kernel<64,16>", 64, 19, 37), ("dwpair_march_kernel<32,32>", 96, 40, 64)])
def test_pair_image_is_independent_of_its_neighbours(kern, C, H, W):
    """also the pair's tensor-wide buffer descriptors: a row index outside image b's rows addresses a neighbour's rows, which are inside the descriptor"""
    assert U.dwconv_pair_route(1, H, W, C)["kernel"] == kern and U.dwconv_pair_route(3, H, W, C)["kernel"] == kern
    x, w3, b3, w7, b7 = U.exact_inputs_pair(1, C, H, W, 3)
    g = U.gen(C, H, W, 98)
    alone = _pair(x, w3, b3, w7, b7)
    three = _pair(torch.cat([_big(x.shape, g), x.float(), _big(x.shape, g)], 0), w3, b3, w7, b7)
    xp_ref = U.conv_int(x, w3, b3, 3, 1, 1)
    for name, a, t3, ref in (("x'", alone[0], three[0], xp_ref), ("t", alone[1], three[1], U.conv_int(xp_ref, w7, b7, 7, 1, 1))):
        assert bool(torch.isfinite(t3).all())
        assert torch.equal(U.bits16(t3[1:2]), U.bits16(a)), f"{kern}: {name} of the middle image depends on its neighbours"
        U.check_exact(a, ref, f"{kern} {name}")


# ================================================================================================ refusals
def _refused(rcs, outs):
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs), rcs
    for (buf, y) in outs:
        assert bool(torch.isnan(y.float()).all()) and _guards_intact(buf, y.numel()), "a refused call wrote to its output"


def test_dwconv_refusals_enqueue_nothing():
    n = 2 * 9 * 14 * 16
    x = torch.ones(n, dtype=torch.bfloat16, device=DEV)
    w, b = torch.ones(49 * 16, dtype=torch.float32, device=DEV), torch.ones(16, dtype=torch.float32, device=DEV)
    out = _out(n)
    f, y = lib().fv_op_dwconv, out[1].data_ptr()
    assert all(U.dwconv_route(*a) is None for a in U.DWCONV_REFUSED)
    rcs = [f(None, w.data_ptr(), b.data_ptr(), y, 2, 9, 14, 8, 3, 1, 1, 0, stream()), f(x.data_ptr(), None, b.data_ptr(), y, 2, 9, 14, 8, 3, 1, 1, 0, stream()),
           f(x.data_ptr(), w.data_ptr(), None, y, 2, 9, 14, 8, 3, 1, 1, 0, stream()), f(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, 2, 9, 14, 8, 3, 1, 1, 0, stream())]
    rcs += [f(x.data_ptr(), w.data_ptr(), b.data_ptr(), y, B, H, W, C, k, s, m, 0, stream()) for (B, H, W, C, k, s, m) in U.DWCONV_REFUSED]
    _refused(rcs, [out])


def test_dwconv_mfma_refusals_enqueue_nothing():
    n = 2 * 16 * 16 * 40
    x, tab, b = torch.ones(n, dtype=torch.bfloat16, device=DEV), torch.ones(4 * 7 * 3 * 256, dtype=torch.bfloat16, device=DEV), torch.ones(64, dtype=torch.float32, device=DEV)
    out = _out(n)
    assert all(U.dwconv_mfma_route(*a) is None for a in U.MFMA_REFUSED)
    rcs = [lib().fv_op_dwconv_mfma(x.data_ptr(), tab.data_ptr(), b.data_ptr(), out[1].data_ptr(), B, H, W, C, k, 0, stream()) for (B, H, W, C, k) in U.MFMA_REFUSED]
    _refused(rcs, [out])


def test_dwconv_s2_refusals_enqueue_nothing():
    n = 2 * 17 * 16 * 96
    x, tab, b = torch.ones(n, dtype=torch.bfloat16, device=DEV), torch.ones(3 * 2 * 7 * 4 * 256, dtype=torch.bfloat16, device=DEV), torch.ones(96, dtype=torch.float32, device=DEV)
    out = _out(n)
    assert all(U.dwconv_s2_route(*a, _cus()) is None for a in U.S2_REFUSED)
    rcs = [lib().fv_op_dwconv_s2_mfma(x.data_ptr(), tab.data_ptr(), b.data_ptr(), out[1].data_ptr(), B, H, W, C, 0, stream()) for (B, H, W, C) in U.S2_REFUSED]
    _refused(rcs, [out])


def test_dwconv_pair_refusals_enqueue_nothing():
    n = 2 * 16 * 32 * 48
    x = torch.ones(n, dtype=torch.bfloat16, device=DEV)
    t3, t7 = torch.ones(3 * 3 * 2 * 256, dtype=torch.bfloat16, device=DEV), torch.ones(3 * 7 * 3 * 256, dtype=torch.bfloat16, device=DEV)
    b3, b7 = torch.ones(64, dtype=torch.float32, device=DEV), torch.ones(64, dtype=torch.float32, device=DEV)
    o1, o2 = _out(n), _out(n)
    f = lambda xp, y1, y2, B, H, W, C: lib().fv_op_dwconv_pair(xp, t3.data_ptr(), b3.data_ptr(), t7.data_ptr(), b7.data_ptr(), y1, y2, B, H, W, C, stream())  # noqa: E731
    assert all(U.dwconv_pair_route(*a) is None for a in U.PAIR_REFUSED) and U.dwconv_pair_route(2, 16, 32, 32) is not None
    rcs = [f(x.data_ptr(), o1[1].data_ptr(), o2[1].data_ptr(), B, H, W, C) for (B, H, W, C) in U.PAIR_REFUSED]
    rcs += [f(o1[1].data_ptr(), o1[1].data_ptr(), o2[1].data_ptr(), 2, 16, 32, 32),      # x == y1
            f(x.data_ptr(), o1[1].data_ptr(), o1[1].data_ptr(), 2, 16, 32, 32)]          # y1 == y2
    _refused(rcs, [o1, o2])
