"""CPU: the references, route mirror and case tables behind tests/test_gpu_dw_backward.py (tests/dw_bwd_util.py).

* the int64 references (written from the definition, one scatter / gather per tap) agree EXACTLY with the float64 torch.autograd references on the integer inputs
  of the exact class, for all five (k, stride, mult) instances, both stride-2 parities, with and without a residual;
* the case tables cover every (route x instance) pair the route mirror says is reachable, each case sits on the route it names, at most MAX_UNREACHABLE pairs are
  listed as unreachable (none is), and every listed one names the condition that excludes it;
* the exactness budgets hold for every case, computed from the case's own sizes: input-gradient sums stay below 2048 (exact in fp16), tap-gradient sums below 2^24
  (exact in fp32 whatever the summation order);
* the scratch size the mirror restates covers the partial-sum rows of whichever route a shape takes (the LDS-staged route's were not covered before this file)."""
import itertools

import pytest
import torch

import dw_bwd_util as U


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g)


@pytest.mark.parametrize("k,stride,mult", U.INSTANCES)
@pytest.mark.parametrize("Hi,Wi", [(9, 14), (10, 13), (11, 17), (4, 5)])
def test_integer_references_equal_float64_autograd(k, stride, mult, Hi, Wi):
    g = torch.Generator().manual_seed(k * 1000 + stride * 100 + mult * 10 + Hi)
    B, Ci = 2, 8
    Co, Ho, Wo = Ci * mult, U.out_size(Hi, k, stride), U.out_size(Wi, k, stride)
    x, dy = _ints((B, Ci, Hi, Wi), -4, 4, g), _ints((B, Co, Ho, Wo), -4, 4, g)
    w, res = _ints((k * k, Co), -3, 3, g), _ints((B, Ci, Hi, Wi), -512, 512, g)
    for r in (None, res):
        got = U.dgrad_int(dy, w, r, Hi, Wi, k, stride, mult)
        ref = U.dgrad_ref(dy, w, r, Hi, Wi, k, stride, mult)
        assert got.dtype == torch.int64 and torch.equal(got.double(), ref)
        assert int(got.abs().max()) <= U.dgrad_bound(k, mult, r is not None) < 2048
    dw, db = U.wgrad_int(x, dy, k, stride, mult)
    rw, rb = U.wgrad_ref(x, dy, k, stride, mult)
    assert dw.dtype == torch.int64 and torch.equal(dw.double(), rw) and torch.equal(db.double(), rb)
    assert int(dw.abs().max()) <= U.wgrad_bound(B, Ho, Wo)


def test_stride2_leaves_input_positions_without_output():
    """what the (9, 14) / (10, 13) maps are for: under the 3x3 stride-2 conv an even-sized side ends in an input row / column that only the last output touches through its
    outermost tap, and a single dy element reaches every second input position only -- the parity skip of dw_dgrad_kernel decides which"""
    for Hi, Wi in [(9, 14), (10, 13)]:
        Ho, Wo = U.out_size(Hi, 3, 2), U.out_size(Wi, 3, 2)
        assert (Ho, Wo) == ((Hi + 1) // 2, (Wi + 1) // 2)
        dy = torch.zeros(1, 8, Ho, Wo, dtype=torch.int64)
        dy[0, :, Ho - 1, Wo - 1] = 1
        w = torch.arange(1, 10).view(9, 1).repeat(1, 8)
        dx = U.dgrad_int(dy, w, None, Hi, Wi, 3, 2, 1)
        ys, xs = torch.nonzero(dx[0, 0], as_tuple=True)
        assert int(ys.min()) == 2 * (Ho - 1) - 1 and int(xs.min()) == 2 * (Wo - 1) - 1
        assert int(ys.max()) == min(Hi - 1, 2 * (Ho - 1) + 1) and int(xs.max()) == min(Wi - 1, 2 * (Wo - 1) + 1)


def test_flipped_table_is_the_table_of_the_mirrored_taps():
    g = torch.Generator().manual_seed(3)
    for k in (3, 7):
        w = _ints((k * k, 32), -3, 3, g).float()
        t, tn = U.toeplitz_flipped16(w, k), U.toeplitz_flipped16(w, k, flip=False)
        assert t.dtype == torch.float16 and t.shape == (2, k, (k + 6) // 4, 16, 4, 4)
        # entry [g][ky][m][ch][i][kk] = flipped[ky][4m + kk - i] = w[k-1-ky][k-1-(4m + kk - i)]
        wv = w.t().reshape(32, k, k)
        for (gi, ky, m, ch, i, kk) in [(0, 0, 0, 0, 0, 0), (1, k - 1, 1, 5, 3, 2), (0, 1, 0, 15, 1, 3), (1, 2, 1, 9, 2, 0)]:
            kx = 4 * m + kk - i
            want = float(wv[gi * 16 + ch, k - 1 - ky, k - 1 - kx]) if 0 <= kx < k else 0.0
            assert float(t[gi, ky, m, ch, i, kk]) == want
        assert not torch.equal(t, tn)


def test_dgrad_cases_cover_every_instance_map_and_channel_count():
    assert {c[:3] for c in U.DGRAD_CASES} == set(U.INSTANCES)
    for inst in U.INSTANCES:
        maps = {(c[4], c[5]) for c in U.DGRAD_CASES if c[:3] == inst}
        assert maps == ({(9, 14), (10, 13)} if inst[1] == 2 else {(11, 17)}), inst
    assert {c[3] for c in U.DGRAD_CASES} == {8, 24, 96, 160, 256}
    assert (7, 2, 2, 96) in {c[:4] for c in U.DGRAD_CASES} or (3, 1, 2, 96) in {c[:4] for c in U.DGRAD_CASES}
    for (k, s, m, Ci, Hi, Wi) in U.DGRAD_CASES:
        assert U.dgrad_route(2, Hi, Wi, Ci, k, s, m) == f"dw_dgrad_kernel<{k},{s},{m}>"
        assert U.dgrad_bound(k, m, True) < 2048
    # the slab logic the channel counts were chosen for
    assert U.dgrad_geometry(8, 1) == {"CS": 8, "nslabs": 1, "G": 1, "ppb": 256, "idle": 0}
    assert U.dgrad_geometry(24, 1) == {"CS": 24, "nslabs": 1, "G": 3, "ppb": 85, "idle": 1}
    assert U.dgrad_geometry(96, 1)["G"] == 12 and U.dgrad_geometry(96, 1)["nslabs"] == 1
    assert U.dgrad_geometry(160, 1)["nslabs"] == 2 and U.dgrad_geometry(256, 1)["nslabs"] == 2
    assert U.dgrad_geometry(96, 2)["CS"] == 48 and U.dgrad_geometry(96, 2)["nslabs"] == 2


def test_mfma_dgrad_cases_and_refusals():
    assert {c[0] for c in U.DGRAD_MFMA_CASES} == {3, 7}
    for (k, C, H, W) in U.DGRAD_MFMA_CASES:
        assert U.dgrad_mfma_route(2, H, W, C, k) == f"dwconv_march_kernel<{k},GRAD>"
        assert U.tower_dgrad_route(2, H, W, C, k, 1, 1) == f"dwconv_march_kernel<{k},GRAD>"   # the route the tower's backward takes for such a layer
        assert U.dgrad_route(2, H, W, C, k, 1, 1) == f"dw_dgrad_kernel<{k},1,1>"              # and the same inputs have a VALU instance to be compared with
        assert U.dgrad_bound(k, 1, True) < 2048
    strips = {((W + 31) // 32, W % 32) for (_, _, _, W) in U.DGRAD_MFMA_CASES}
    assert (1, 16) in strips and (2, 1) in strips and (3, 6) in strips and any(H % 8 for (_, _, H, _) in U.DGRAD_MFMA_CASES)
    for (k, C, H, W) in U.DGRAD_MFMA_REFUSED:
        assert U.dgrad_mfma_route(2, H, W, C, k) is None


def test_wgrad_cases_cover_every_reachable_pair_and_stay_exact():
    covered = set()
    for (route, k, s, m, Ci, Hi, Wi, B) in U.WGRAD_CASES:
        assert U.wgrad_route(B, Hi, Wi, Ci, k, s, m) == route, (route, U.wgrad_route(B, Hi, Wi, Ci, k, s, m))
        Ho, Wo = U.out_size(Hi, k, s), U.out_size(Wi, k, s)
        assert U.wgrad_bound(B, Ho, Wo) < 2 ** 24
        rows = U.wgrad_part_rows(B, Hi, Wi, Ci, k, s, m)
        assert rows * (k * k + 1) * Ci * m <= U.wgrad_scratch_floats(B, Ho, Wo, Ci * m, k)
        covered.add(route)
    covered |= {f"dwconv_march_kernel<{k},GRAD>" for (k, _, _, _) in U.DGRAD_MFMA_CASES}
    assert {c[7] for c in U.WGRAD_CASES} >= {1, 3}
    assert len(U.UNREACHABLE) <= U.MAX_UNREACHABLE and all(p in U.ALL_PAIRS and cond for p, cond in U.UNREACHABLE.items())
    assert covered | set(U.UNREACHABLE) == set(U.ALL_PAIRS), sorted(set(U.ALL_PAIRS) - covered - set(U.UNREACHABLE))
    assert not covered & set(U.UNREACHABLE)


def test_route_mirror_reaches_every_pair_and_scratch_covers_every_route():
    """a sweep of small shapes: every pair of ALL_PAIRS that is not listed unreachable IS reached by some shape (the table above is not the only witness), and the
    partial-sum rows of the route taken always fit dw_bwd_scratch_floats"""
    seen = set()
    for (k, s, m), Ci, B, Hi, Wi in itertools.product(U.INSTANCES, (8, 24, 32, 48, 64, 96, 160, 384), (1, 2, 3, 32), (6, 9, 16, 17, 18, 33), (6, 12, 16, 20, 33, 34, 70)):
        r = U.wgrad_route(B, Hi, Wi, Ci, k, s, m)
        seen.add(r)
        Ho, Wo = U.out_size(Hi, k, s), U.out_size(Wi, k, s)
        assert U.wgrad_part_rows(B, Hi, Wi, Ci, k, s, m) * (k * k + 1) * Ci * m <= U.wgrad_scratch_floats(B, Ho, Wo, Ci * m, k), (r, B, Hi, Wi, Ci)
        if s == 1 and m == 1:
            seen.add(U.dgrad_mfma_route(B, Hi, Wi, Ci, k))
    seen.discard(None)
    assert seen == set(U.ALL_PAIRS) - set(U.UNREACHABLE)
