"""CPU checks of what tests/test_gpu_dw_forward.py relies on (tests/dw_fwd_util.py): the int64 references against float64 conv2d, the stride-2 Toeplitz helper
against its definition, the route mirror against the case tables (every reachable instance has a case on the route it names; exactly four compiled instances are
unreachable), the exact class's budgets, the GELU functions' documented errors -- and the checks themselves against a float32 / bf16 emulation of the kernels'
arithmetic with defects planted: each defect fails the check meant to catch it, two of them pass the tolerance the forward op tests had before
(gpu_util.check_close at its defaults), and the clean emulation passes everything."""
import pytest
import torch

import dw_fwd_util as U
from gpu_util import check_close

CUS = 256      # the MI355X's compute units: the stride-2 mirror is evaluated for them here, and for the device's own count on the GPU


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("k,stride,mult,H,W", [(k, s, m, H, W) for (k, s, m) in U.INSTANCES for (H, W) in U.VALU_MAPS[s]] + [(7, 1, 1, 19, 33), (3, 1, 1, 17, 40), (7, 2, 2, 18, 34)])
def test_int_reference_equals_float64_conv2d(k, stride, mult, H, W):
    """every instance, both parities of the stride-2 maps (9 x 14, 10 x 13), a map narrower than the window (5 x 3)"""
    x, w, b = U.exact_inputs(2, 16, H, W, k, stride, mult)
    ref = U.conv_int(x, w, b, k, stride, mult)
    f64 = U.conv_f64(x, w, b, k, stride, mult)
    assert ref.shape == f64.shape == (2, 16 * mult, U.out_size(H, k, stride), U.out_size(W, k, stride))
    assert torch.equal(ref.double(), f64)
    assert int(ref.abs().max()) <= U.exact_budget(k) <= U.EXACT_LIMIT
    assert int(ref.abs().max()) > U.exact_budget(k) // 8          # the inputs do use the range


def test_int_reference_of_the_pair():
    x, w3, b3, w7, b7 = U.exact_inputs_pair(2, 32, 19, 37)
    assert bool((b3 != 0).all()) and int(b3.abs().max()) == 2 and bool(((w7 != 0).sum((1, 2, 3)) == U.PAIR_TAPS7).all())
    xp = U.conv_int(x, w3, b3, 3, 1, 1)
    t = U.conv_int(xp, w7, b7, 7, 1, 1)
    assert torch.equal(xp.double(), U.conv_f64(x, w3, b3, 3, 1, 1)) and torch.equal(t.double(), U.conv_f64(xp, w7, b7, 7, 1, 1))
    mx, mt = U.exact_budget_pair()
    assert int(xp.abs().max()) <= mx and int(t.abs().max()) <= mt <= U.EXACT_LIMIT
    # x' outside the map is the 7x7's ZERO padding: with the 3x3's bias there instead, t differs (b3 is non-zero in every channel)
    _, t_b3 = U.emulate_pair(x, w3, b3, w7, b7, pad_b3=True)
    assert not torch.equal(t_b3.double(), t.double())


def test_toeplitz_s2_matches_its_definition():
    w = torch.arange(2 * 32 * 49, dtype=torch.float32).view(64, 1, 7, 7) + 1.0           # every tap distinct and non-zero
    got, want = U.toeplitz_s2(w), U.toeplitz_s2_definition(w)
    assert got.shape == want.shape == (2, 2, 7, 4, 16, 4, 4) and torch.equal(got, want)
    assert int((want != 0).sum()) == 2 * 2 * 7 * 16 * sum(1 for m in range(4) for i in range(4) for kk in range(4) if 0 <= 4 * m + kk - 2 * i < 7)
    # and the stride-1 table the other MFMA routes take, one element at a time: [C/16][k][NM][16][4 i][4 kk] = w[ky][4m + kk - i]
    for k in (3, 7):
        w1 = torch.arange(32 * k * k, dtype=torch.float32).view(32, 1, k, k) + 1.0
        t = U.toeplitz(w1, k)
        nm = (k + 6) // 4
        assert t.shape == (2, k, nm, 16, 4, 4)
        for (g, ky, m, ch, i, kk) in [(0, 0, 0, 0, 0, 0), (1, k - 1, nm - 1, 15, 3, 3), (1, 1, 1, 7, 2, 1), (0, k // 2, 0, 3, 3, 0), (0, 2, nm - 1, 9, 0, 3)]:
            kx = 4 * m + kk - i
            assert float(t[g, ky, m, ch, i, kk]) == (float(w1[16 * g + ch, 0, ky, kx]) if 0 <= kx < k else 0.0)


# ------------------------------------------------------------------------------------------------ routes and tables
def test_every_reachable_instance_has_cases_on_its_route():
    covered = set()
    for (k, s, m, Ci, H, W) in U.VALU_CASES:
        r = U.dwconv_route(2, H, W, Ci, k, s, m)
        assert r["kernel"] == f"dwconv_kernel<{k},{s},{m}>"
        covered.add(r["kernel"])
    for (k, C, H, W) in U.TILE_CASES:
        r = U.dwconv_route(2, H, W, C, k, 1, 1)
        assert r["kernel"] == f"dwconv_tile_kernel<{k}>"
        covered.add(r["kernel"])
    for (kern, k, C, H, W) in U.MFMA_CASES:
        assert U.dwconv_mfma_route(2, H, W, C, k)["kernel"] == kern
        covered.add(kern)
    for (C, H, W, B) in U.S2_CASES:
        covered.add(U.dwconv_s2_route(B, H, W, C, CUS)["kernel"])
    for (kern, C, H, W, B, nseg) in U.PAIR_CASES:
        r = U.dwconv_pair_route(B, H, W, C)
        assert r["kernel"] == kern and r["nseg"] == nseg
        covered.add(kern)
    assert covered == set(U.REACHABLE) and len(U.REACHABLE) == 13


def test_the_unreachable_instances_are_exactly_four():
    assert sorted(U.UNREACHABLE) == ["dwconv_march_kernel<3>", "dwconv_mfma_kernel<7,16>", "dwpair_march_kernel<32,16>", "dwpair_march_kernel<64,8>"]
    assert not set(U.UNREACHABLE) & set(U.REACHABLE) and all(U.UNREACHABLE.values())
    # no shape reaches them: a sweep of the mirrors over shapes on both sides of every threshold names only reachable kernels
    seen = set()
    for C in (8, 24, 32, 64, 96, 128):
        for H in (2, 8, 15, 16, 31, 32, 33, 64):
            for W in (3, 15, 16, 31, 32, 33, 64):
                for (k, s, m) in U.INSTANCES:
                    r = U.dwconv_route(2, H, W, C, k, s, m)
                    seen |= {r["kernel"]} if r else set()
                for k in (3, 7):
                    r = U.dwconv_mfma_route(2, H, W, C, k)
                    seen |= {r["kernel"]} if r else set()
                for r in (U.dwconv_s2_route(2, H, W, C, CUS), U.dwconv_pair_route(2, H, W, C)):
                    seen |= {r["kernel"]} if r else set()
    assert seen == set(U.REACHABLE)


def test_valu_cases_vary_the_slice_rule_and_the_last_quad():
    """GS = the largest divisor <= 16 of C mult / 8: one group (GS 1, one slice), 3, 17 = prime (GS 1, 17 slices), 20 (GS 10, two slices, 6 idle threads), and their
    doubles under mult 2; no output row is a whole number of quads"""
    geo = {(m, Ci): U.dwconv_route(2, H, W, Ci, k, s, m) for (k, s, m, Ci, H, W) in U.VALU_CASES}
    assert {(m, Ci): (r["GS"], r["nslices"]) for (m, Ci), r in geo.items()} == {(1, 8): (1, 1), (1, 24): (3, 1), (1, 136): (1, 17), (1, 160): (10, 2),
                                                                                  (2, 8): (2, 1), (2, 24): (6, 1), (2, 136): (2, 17), (2, 160): (10, 4)}
    assert geo[(1, 160)]["idle"] == 6 and geo[(1, 24)]["idle"] == 1
    assert all(U.dwconv_route(2, H, W, Ci, k, s, m)["last_quad"] != 0 for (k, s, m, Ci, H, W) in U.VALU_CASES)
    assert {(s, H % 2, W % 2) for (k, s, m, Ci, H, W) in U.VALU_CASES if s == 2} == {(2, 1, 0), (2, 0, 1)}
    assert len(U.VALU_CASES) == 5 * 4 * 2


def test_mfma_cases_cover_ragged_tiles_half_strips_and_the_ring():
    tile = [U.dwconv_route(2, H, W, C, k, 1, 1) for (k, C, H, W) in U.TILE_CASES if k == 7]
    assert [(r["tiles_x"], r["tiles_y"], r["nsl"]) for r in tile] == [(1, 1, 1), (2, 3, 2), (3, 2, 3)]
    march = [(H, W, U.dwconv_mfma_route(2, H, W, C, k)) for (kern, k, C, H, W) in U.MFMA_CASES if kern == "dwconv_march_kernel<7>"]
    assert [r["groups"] for (_, _, r) in march] == [2, 3, 3, 6] and march[-1][0] % 8 == 1          # six groups: the 16-row ring wraps twice; the last group is one row
    assert any(W == 16 for (_, W, _) in march) and any(r["tiles_x"] == 3 for (_, _, r) in march)
    for kern in ("dwconv_mfma_kernel<7,8>", "dwconv_mfma_kernel<3,8>"):
        ws = [W for (kn, k, C, H, W) in U.MFMA_CASES if kn == kern]
        assert any(W <= 20 for W in ws) and any(W > 32 for W in ws)                               # a half-masked strip, and a second strip
    assert all(H < 16 for (kn, k, C, H, W) in U.MFMA_CASES if kn == "dwconv_mfma_kernel<7,8>")


def test_the_stride2_walking_case_walks_at_256_cus():
    C, H, W, B = U.S2_WALK_CASE
    r = U.dwconv_s2_route(B, H, W, C, CUS)
    assert (r["chains"], r["tpx"], r["tiles"], r["nsl"]) == (2, 5, 36, 32) and r["tpx"] > r["chains"]
    p = U.dwconv_s2_walk_properties(B, H, W, C, CUS)
    assert p["longest"] >= 3 and p["crosses_images"] and p["last_xcd_short"] and p["complete"] and r["tiles"] % 8 != 0
    assert B * H * W * C * 2 < 64 * 2 ** 20
    # the other shapes give every block at most one tile -- as every shape of test_dwconv_s2_mfma does (the hole this case closes)
    for (C2, H2, W2, B2) in U.S2_CASES[:-1] + [(32, 16, 32, 2), (192, 32, 32, 2)]:
        q = U.dwconv_s2_walk_properties(B2, H2, W2, C2, CUS)
        assert q["longest"] == 1 and q["complete"]
    # whatever the CU count, every tile is visited exactly once
    for cus in (1, 8, 64, 104, 256, 304):
        assert U.dwconv_s2_walk_properties(B, H, W, C, cus)["complete"] and U.dwconv_s2_walk_properties(2, 40, 64, 96, cus)["complete"]


def test_pair_cases_cut_and_uncut():
    routes = [(c, U.dwconv_pair_route(c[4], c[2], c[3], c[1])) for c in U.PAIR_CASES]
    for geo in ("dwpair_march_kernel<64,16>", "dwpair_march_kernel<32,32>"):
        uncut = [(c, r) for (c, r) in routes if c[0] == geo and r["nstrips"] >= 256]
        assert len(uncut) == 1 and uncut[0][1]["nseg"] == 1 and uncut[0][1]["groups"] >= 4
        c = uncut[0][0]
        assert U.dwconv_pair_route(c[4] - 1, c[2], c[3], c[1])["nstrips"] < 256                   # the smallest B the launcher walks uncut
        assert any(r["nseg"] > 1 and r["cut_to_half"] for (c2, r) in routes if c2[0] == geo)
    assert any(r["nseg"] == 3 and r["starts"] == [0, 2, 4] for (_, r) in routes)                  # a segment of two groups and one of three
    assert {r["geometry"] for (_, r) in routes} == {(64, 16), (32, 32)}
    assert all(c[4] * c[1] * c[2] * c[3] * 2 < 64 * 2 ** 20 for c in U.PAIR_CASES)


def test_refused_shapes_are_refused_by_the_mirror():
    assert all(U.dwconv_route(*a) is None for a in U.DWCONV_REFUSED)
    assert all(U.dwconv_mfma_route(*a) is None for a in U.MFMA_REFUSED)
    assert all(U.dwconv_s2_route(*a, CUS) is None for a in U.S2_REFUSED)
    assert all(U.dwconv_pair_route(*a) is None for a in U.PAIR_REFUSED)


def test_exact_budgets_fit_bf16():
    """each class's largest possible |output| from its own sizes: 49 x 2 x 1 + 8, 9 x 8 x 3 + 8, and for the pair |x'| <= 9 + 2, |t| <= 20 x 11 + 8"""
    assert U.exact_budget(7) == 106 and U.exact_budget(3) == 224 and U.exact_budget_pair() == (11, 228)
    assert max(U.exact_budget(7), U.exact_budget(3), *U.exact_budget_pair()) <= U.EXACT_LIMIT
    v = torch.arange(-U.EXACT_LIMIT, U.EXACT_LIMIT + 1, dtype=torch.float32)
    assert torch.equal(v.to(torch.bfloat16).float(), v)                                           # every integer of the budget is a bf16 value
    assert int(U.selection_taps(64, 7).max()) == 53 and torch.equal(U.bf16_round(U.selection_taps(64, 7)), U.selection_taps(64, 7).float())


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("k,stride,mult,H,W", [(7, 1, 1, 19, 33), (3, 1, 1, 17, 40), (7, 2, 2, 18, 34), (3, 2, 1, 9, 14), (7, 2, 2, 10, 13), (3, 1, 2, 5, 3)])
def test_selection_expected_is_the_convolution_of_the_impulses(k, stride, mult, H, W):
    C = 8
    pos = U.selection_positions(H, W, U.boundary_pairs(8, H, limit=2), U.boundary_pairs(32, W))
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)} <= set(pos)
    images = U.pack_positions(pos, k)
    assert sorted(p for im in images for p in im) == sorted(pos)
    x, w = U.selection_input(images, C, H, W), U.selection_taps(C * mult, k)
    want = U.selection_expected(images, w, H, W, k, stride, mult)
    assert torch.equal(want, U.conv_int(x, w, torch.zeros(C * mult, dtype=torch.int64), k, stride, mult))
    if stride == 2:
        assert {(r % 2, c % 2) for (r, c) in pos} == {(0, 0), (0, 1), (1, 0), (1, 1)}            # impulses at even and at odd coordinates
    # an interior impulse of a stride-1 map shows the whole mirrored patch: output (r + pad - ky, c + pad - kx) holds tap (ky, kx)
    if stride == 1 and H > k and W > k:
        b = next(i for i, im in enumerate(images) if (H // 2, W // 2) in im)
        patch = want[b, 3, H // 2 - k // 2:H // 2 + k // 2 + 1, W // 2 - k // 2:W // 2 + k // 2 + 1]
        assert torch.equal(patch, torch.flip(w[3, 0], dims=[0, 1]))


# ------------------------------------------------------------------------------------------------ GELU
@pytest.mark.parametrize("name", sorted(U.GELU_ERR))
def test_gelu_emulations_hold_their_documented_error(name):
    """a float32 emulation of each function on a grid over [-9, 9] against the erf form in float64: the documented maximum holds, and is not slack by more than a
    quarter (a bound that loose would hide a wrong coefficient)"""
    x = torch.linspace(-9.0, 9.0, 2 ** 21 + 1, dtype=torch.float64).to(torch.float32)
    err = float((U.GELU_EMULATED[name](x).double() - U.gelu_erf(x)).abs().max())
    print(f"[dw-fwd gelu] {name}: max |error| = {err:.4e} (documented {U.GELU_ERR[name]:.2e})")
    assert 0.75 * U.GELU_ERR[name] <= err <= U.GELU_ERR[name]
    assert float(U.gelu_erf(torch.tensor([2.0 ** 0.5])).item()) > 0 and U.GELU_SLOPE >= 1.1290   # max gelu' = Phi + x phi at x = sqrt 2


# ------------------------------------------------------------------------------------------------ the checks against planted defects
def _fails(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def test_the_checks_tell_the_broken_arithmetics():
    """C = 64, 19 x 33, k = 7, the suite's Gaussian recipe.  Truncation and an un-rounded x' pass check_close at its defaults -- the gap -- and fail the per-element
    bound; a bias in the pair's padding and a zeroed Toeplitz slot fail the exact class."""
    B, C, H, W, k = 2, 64, 19, 33, 7
    x, w, b = U.gauss_inputs(B, C, H, W, k, 1, 1, table=True)
    pre, A = U.conv_f64(x, w, b, k, 1, 1), U.conv_abs(x, w, b, k, 1, 1)
    # 1. the output truncated to bf16 instead of rounded
    clean, trunc = U.emulate_conv(x, w, b, k, 1, 1), U.emulate_conv(x, w, b, k, 1, 1, truncate=True)
    U.check_gauss(clean, pre, A, k, what="clean 7x7")
    check_close(clean, pre.float(), what="clean 7x7")
    # the rounding term is bf16's half-ulp AT the value: with 2^-9 |ref| in its place (the half-ulp relative to the top of a binade) correct rounding itself is
    # over, by up to 2 just above a power of two; truncation is over the half-ulp form by up to 2 and over this one by up to 4
    lit_clean, lit_trunc = U.gauss_fraction(clean, pre, A, k, literal=True)[0], U.gauss_fraction(trunc, pre, A, k, literal=True)[0]
    assert 1.9 < lit_clean <= 2.0 and U.gauss_fraction(clean, pre, A, k)[0] > 0.95 and 3.8 < lit_trunc <= 4.0 and 1.9 < U.gauss_fraction(trunc, pre, A, k)[0] <= 2.0
    check_close(trunc, pre.float(), what="truncated 7x7")                                         # passes: rel-L2 3e-3 against 4e-3
    assert _fails(U.check_gauss, trunc, pre, A, k, what="truncated 7x7")
    for gelu in sorted(U.GELU_ERR):
        U.check_gauss(U.emulate_conv(x, w, b, k, 1, 1, gelu=gelu), pre, A, k, gelu, what=f"clean 7x7 {gelu}")
        assert _fails(U.check_gauss, U.emulate_conv(x, w, b, k, 1, 1, gelu=gelu, truncate=True), pre, A, k, gelu, what=f"truncated 7x7 {gelu}")
    # 2. the pair's 7x7 fed the un-rounded x'
    x, w3, b3 = U.gauss_inputs(B, C, H, W, 3, 1, 1, 5, table=True)
    _, w7, b7 = U.gauss_inputs(B, C, H, W, 7, 1, 1, 6, table=True)

    def pair_checks(xp, t, what):
        U.check_gauss(xp, U.conv_f64(x, w3, b3, 3, 1, 1), U.conv_abs(x, w3, b3, 3, 1, 1), 3, what=what + " x'")
        U.check_gauss(t, U.conv_f64(xp, w7, b7, 7, 1, 1), U.conv_abs(xp, w7, b7, 7, 1, 1), 7, what=what + " t")      # against the x' that was RETURNED

    xp, t = U.emulate_pair(x, w3, b3, w7, b7)
    pair_checks(xp, t, "clean pair")
    xp_u, t_u = U.emulate_pair(x, w3, b3, w7, b7, unrounded=True)
    assert torch.equal(xp_u, xp) and not torch.equal(t_u, t)
    ref1 = U.bf16_round(U.conv_f64(x, w3, b3, 3, 1, 1).float())
    check_close(xp_u, ref1, what="un-rounded pair x'")
    check_close(t_u, U.conv_f64(ref1, w7, b7, 7, 1, 1).float(), what="un-rounded pair t")         # passes: what test_dwconv_pair asserts
    assert _fails(pair_checks, xp_u, t_u, "un-rounded pair")
    # 3. x' outside the map equal to b3; 4. one Toeplitz slot of one strip column zeroed: the exact class
    xi, w3i, b3i, w7i, b7i = U.exact_inputs_pair(B, C, H, W)
    xpi = U.conv_int(xi, w3i, b3i, 3, 1, 1)
    ti = U.conv_int(xpi, w7i, b7i, 7, 1, 1)
    xp_e, t_e = U.emulate_pair(xi, w3i, b3i, w7i, b7i)
    U.check_exact(xp_e, xpi, "clean pair x'")
    U.check_exact(t_e, ti, "clean pair t")
    xp_p, t_p = U.emulate_pair(xi, w3i, b3i, w7i, b7i, pad_b3=True)
    U.check_exact(xp_p, xpi, "padded-with-b3 pair x'")
    assert _fails(U.check_exact, t_p, ti, "padded-with-b3 pair t")
    assert torch.equal(t_p[:, :, 3:-3, 3:-3].double(), ti[:, :, 3:-3, 3:-3].double())             # only the border rows and columns see it
    xe, we, be = U.exact_inputs(B, C, H, W, k, 1, 1)
    ref = U.conv_int(xe, we, be, k, 1, 1)
    U.check_exact(U.emulate_conv(xe, we, be, k, 1, 1), ref, "clean exact 7x7")
    ch = next(c for c in range(C) if int(we[c, 0, 2, 2]) != 0)
    slot = U.emulate_conv(xe, we, be, k, 1, 1, zero_slot=(ch, 2, 2, 32))                           # column 32: the first of the second strip
    assert _fails(U.check_exact, slot, ref, "zeroed slot, exact")
    assert 0 < int((slot.double() != ref.double()).sum()) <= B * H                                # one column of one channel
    # the Gaussian class does not miss it either, and the selection class sees it wherever an impulse's patch covers the column (31 | 32 is a strip boundary)
    assert _fails(U.check_gauss, U.emulate_conv(x, w, b, k, 1, 1, zero_slot=(5, 2, 2, 32)), pre, A, k, what="zeroed slot, Gaussian")
    images = U.pack_positions(U.selection_positions(H, W, U.boundary_pairs(8, H, limit=2), U.boundary_pairs(32, W)), k)
    xs, ws = U.selection_input(images, C, H, W), U.selection_taps(C, k)
    want = U.selection_expected(images, ws, H, W, k, 1, 1)
    zb = torch.zeros(C, dtype=torch.int64)
    U.check_bits(U.emulate_conv(xs, ws, zb, k, 1, 1), want, "clean selection")
    assert _fails(U.check_bits, U.emulate_conv(xs, ws, zb, k, 1, 1, zero_slot=(5, 2, 2, 32)), want, "zeroed slot, selection")


@pytest.mark.parametrize("k,stride,mult,C,H,W", [(3, 1, 1, 24, 11, 17), (7, 2, 2, 24, 10, 13), (3, 2, 1, 8, 9, 14), (3, 1, 2, 8, 5, 3), (7, 1, 1, 32, 24, 70), (3, 1, 1, 32, 16, 20)])
def test_the_clean_emulation_passes_every_check(k, stride, mult, C, H, W):
    """so the Gaussian inputs are ones for which float32 arithmetic with one bf16 rounding stays inside the bound, GELU included, and the exact class is exact"""
    B = 2
    x, w, b = U.gauss_inputs(B, C, H, W, k, stride, mult, table=(C % 32 == 0))
    pre, A = U.conv_f64(x, w, b, k, stride, mult), U.conv_abs(x, w, b, k, stride, mult)
    fr = [U.check_gauss(U.emulate_conv(x, w, b, k, stride, mult), pre, A, k, what="clean")]
    fr += [U.check_gauss(U.emulate_conv(x, w, b, k, stride, mult, gelu=g), pre, A, k, g, what=f"clean {g}") for g in sorted(U.GELU_ERR)]
    assert max(fr) > 0.5                                                                          # and the bound is not slack: rounding alone uses most of it
    xe, we, be = U.exact_inputs(B, C, H, W, k, stride, mult)
    U.check_exact(U.emulate_conv(xe, we, be, k, stride, mult), U.conv_int(xe, we, be, k, stride, mult), "clean exact")
