"""CPU: the references tests/test_gpu_attention_bwd.py measures the attention backward against (tests/attn_bwd_ref_util.py).

  * the emulations of the two routes' arithmetic stay under attn_bwd_ref_util.CAPS at every case the GPU tests run -- the GPU tests bound a kernel's worst row by
    TWICE the matching emulation's under the same measure, so the caps are what keeps a loose emulation from hiding a wrong kernel;
  * the exact emulation agrees with plain fp32 autograd of the same operator (a wrong formula in the emulation itself shows here);
  * the cases cross the tile, block and record edges, and reach the launcher branches, they stand for."""
import pytest
import torch

import attn_bwd_ref_util as R


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_backward_emulations_stay_under_their_caps(name):
    c = R.CASE_BY_NAME[name]
    r = R.reference(*c.ref_key)
    m = r["emu_measures"]
    print(f"[{name}] form {c.form}: emulation dq {m['dq']:.2e} dk {m['dk']:.2e} dv {m['dv']:.2e} delta {m['delta']:.2e}; cap {c.cap:.1e}")
    assert all(torch.isfinite(t).all() for t in r["emu"]) and all(torch.isfinite(r[k]).all() for k in ("dq64", "dk64", "dv64", "delta64"))
    assert all(0.0 < v <= c.cap for v in m.values()), m


@pytest.mark.parametrize("name", [s.name for s in R.SHAPES])
def test_exact_emulation_agrees_with_fp32_autograd(name):
    """The hand-written backward of form "exact" against torch.autograd through the fp32 form of the forward, under the same measure.  The two differ by fp32
    rounding and by delta, which the emulation takes from the 16-bit forward output as the kernels do (that alone is ~2e-5 on dq / dk): 5e-5."""
    s = R.SHAPE_BY_NAME[name]
    r = R.reference(name, "exact")
    a = R.autograd_f32(r["qkv"], r["dO"], r["table"], s)
    kl = R.key_lens(s)
    got = [R.block_measure(r["emu"][i], a[i], kl, u) for i, u in enumerate((r["unit_dq"], r["unit_dk"], None))]
    print(f"[{name}] exact emulation vs fp32 autograd: dq {got[0]:.2e} dk {got[1]:.2e} dv {got[2]:.2e}")
    assert max(got) <= 5e-5


def test_delta_from_the_16_bit_output_sets_the_exact_routes_floor():
    """what docs/kernels.md records: with delta from the UN-rounded forward output the exact emulation's dq / dk error is an order of magnitude smaller"""
    r = R.reference("ragged_T150", "exact")
    ideal = R.measures(*R.emulate(r["qkv"], r["dO"], r["table"], r["shape"], "exact", delta_from_rounded_o=False), r)
    m = r["emu_measures"]
    print(f"exact emulation, delta from hi + lo: {m}; from the un-rounded output: {ideal}")
    assert ideal["dq"] < 0.3 * m["dq"] and ideal["dk"] < 0.3 * m["dk"] and ideal["delta"] < 0.3 * m["delta"]


def test_the_backward_cases_cross_the_edges_they_stand_for():
    """the geometry and the routing the case list relies on, restated from launch_attention_bwd / launch_attention_split_bwd and the kernels' block shapes (a
    change there must be followed here)"""
    by = R.CASE_BY_NAME
    sh = R.SHAPE_BY_NAME
    # every case exists on both routes, and every group > 1 with and without part
    for s in R.SHAPES:
        for route in ("split", "fp32"):
            want = ("looped", "parts") if s.heads > s.kv else ("parts",)
            assert all(f"{s.name}-{route}-{p}" in by for p in want), s.name
    # every instance launch_attention_bwd can launch: (route, head_dim, grouped / per-head dq on the split route, PART + reduce / looped)
    seen = {(c.use_split, c.shape.D, c.grouped_dq, c.part_kernels) for c in R.CASES}
    for D in (64, 128):
        for parts in (False, True):
            assert (False, D, False, parts) in seen and (True, D, True, parts) in seen
    assert {(True, 64, False, False), (True, 64, False, True), (True, 128, False, False)} <= seen   # per-head split dq: group 1 (looped only), group 9 (both)
    assert by["no_grouping_T200-split-parts"].group == 1 and not by["no_grouping_T200-split-parts"].part_kernels and by["no_grouping_T200-split-parts"].parts
    assert by["group9_T130-split-parts"].group == 9 and not by["group9_T130-split-parts"].grouped_dq and by["group9_T130-split-parts"].part_kernels
    assert by["group7_T65-split-parts"].group == 7 and by["group7_T65-split-parts"].grouped_dq
    # split route, head_dim 64: blocks of 128 rows, records of 64 keys, steps of 32, grouped dq blocks of 32 queries; fp32 route: blocks of 64
    s = sh["ragged_T150"]
    assert s.T % 128 and s.T % 64 and s.T % 32 and s.T % 16 and R.key_lens(s) == [150, 97] and 97 % 16
    s = sh["one_past_T129"]
    assert s.T % 128 == 1 and s.T % 64 == 1 and s.T % 32 == 1
    s = sh["block_edge"]
    assert R.key_lens(s) == [128, 64] and (s.T + 127) // 128 == 2 and (s.T + 63) // 64 == 3      # key block 1 of 128 (and 64-blocks 1, 2 / 2) lie wholly past len
    assert 1 in R.key_lens(sh["len_one"])
    assert R.key_lens(sh["len_add_40"]) == [45, 60] and R.key_lens(sh["len_add_50_clamps"]) == [55, 60]
    s = sh["engine_Ni64"]
    assert s.len_add == 64 and R.key_lens(s) == [96, 73] and max(s.lens) + s.len_add == s.T
    assert sh["single_token"].T == 1 and sh["one_ragged_tile"].T == 17
    s = sh["group7_T65"]
    assert s.T == 2 * 32 + 1 and s.T == 64 + 1
    assert sh["no_grouping_T200"].T > 128 and sh["group9_T130"].T > 128
    s = sh["d128_T130"]
    assert s.D == 128 and s.T % 64 == 2 and s.T % 16 and R.key_lens(s) == [130, 77] and 77 % 32 and 77 % 16      # NT = 1: 64-row blocks, 16-query grouped blocks
    s = sh["d128_no_grouping_T70"]
    assert s.D == 128 and s.heads == s.kv and 64 < s.T < 128
    assert sh["peaked_T150"].peaked and all(c.cap == R.CAPS[("peaked", c.form)] for c in R.CASES if c.shape.peaked)
    assert all(sp.B <= 3 and sp.T <= 200 for sp in R.SHAPES)
    # the peaked inputs are the plain ones with q and k scaled
    qa, _, _ = R.make_inputs(sh["ragged_T150"])
    qb, _, _ = R.make_inputs(sh["peaked_T150"])
    w = (4 + 2) * 64
    assert torch.equal(qb[..., :w], qa[..., :w] * R.PEAK) and torch.equal(qb[..., w:], qa[..., w:])
    # dO vanishes on the rows >= klen and nowhere else
    for sp in R.SHAPES:
        _, dO, _ = R.make_inputs(sp)
        for b, n in enumerate(R.key_lens(sp)):
            assert bool((dO[b, n:] == 0).all()) and bool((dO[b, :n].abs().sum(-1) > 0).all())
