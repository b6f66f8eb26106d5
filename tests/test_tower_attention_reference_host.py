"""No GPU: the CPU references of tests/tower_attn_ref_util.py, which tests/test_gpu_tower_attention.py measures the bf16 attention kernels (csrc/attention.hip) and the
tower's attention backward (csrc/tower_bwd_kernels.hip tattn_*) against.

The GPU tests bound a kernel's worst row by 2 x the error of the emulation of its arithmetic on the same inputs.  That is only a test if the emulation is tight, so
here every emulation's own measure against float64 is held under a cap at every case and input class (CAPS: conditions, not tolerances).  The rest checks the test
data itself: every case reaches the kernel its name says, the float64 backward agrees with a finite difference, the exact-bit inputs (one-hot selection, constant V)
have the properties the GPU tests assert -- checked by running the same assertions on the emulations -- and the three ways in which the arithmetic could be subtly
different (a swapped key slot in the P.V pairing, an un-rounded row sum in attention32_kernel, delta from the rounded forward output) are each caught by the check that
is meant to catch it."""
import pytest
import torch

import tower_attn_ref_util as R


def test_every_case_reaches_the_kernel_its_name_says():
    """launch_attention's dispatch restated (Case.route) against the table; every instance but attention_kernel<32, false> (behind the tools build's switch) is reached"""
    assert set(R.EXPECTED_ROUTE) == {c.name for c in R.CASES}
    for c in R.CASES:
        assert c.route == R.EXPECTED_ROUTE[c.name], (c.name, c.route)
        assert c.name.startswith("a32_") == (c.route == "attention32_kernel")
    assert {c.route for c in R.CASES} == {"attention32_kernel", "attention_kernel<32, true>", "attention_kernel<64, true>", "attention_kernel<64, false>",
                                          "attention_kernel<128, true>", "attention_kernel<128, false>"}
    assert R.CASE_BY_NAME["gen_len_add_40"].key_lens() == [45, 60] and R.CASE_BY_NAME["gen_len_add_50_clamps"].key_lens() == [55, 60]
    assert R.CASE_BY_NAME["gen_d64_causal_ragged"].key_lens() == [100, 37, 1]


@pytest.mark.parametrize("kind", R.FWD_KINDS)
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_forward_emulation_is_under_its_cap(name, kind):
    r = R.forward_reference(name, kind)
    print(f"[{name} {kind}] emulation worst row {r['emu_measure']:.2e}")
    assert r["emu_measure"] <= R.CAPS["forward"], f"{name} {kind}: {r['emu_measure']:.3e}"
    assert (r["emu_measure"] == 0.0) == (r["case"].T == 1), "one key: the output is v itself, exactly; anywhere else the bf16 rounding must show"
    assert bool(torch.isfinite(r["emu"]).all())


@pytest.mark.parametrize("kind", R.BWD_KINDS)
@pytest.mark.parametrize("name", [c.name for c in R.BWD_CASES])
def test_backward_emulation_is_under_its_caps(name, kind):
    r = R.backward_reference(name, kind)
    m = r["emu_measures"]
    print(f"[{name} {kind}] " + "  ".join(f"{k} {v:.2e}" for k, v in m.items()))
    for k in ("dq", "dk", "dv"):
        assert m[k] <= R.CAPS[(kind, k)], f"{name} {kind}: {k} {m[k]:.3e} over {R.CAPS[(kind, k)]:.1e}"
    # the statistics are fp32: lse2 to a few ulps of its size (|lse2| <= ~600 at the peaked class), delta to fp32 rounding of a sum over T terms
    assert m["lse2"] <= 2e-4 and m["delta"] <= 2e-5, (name, kind, m)


def test_backward_float64_reference_agrees_with_a_finite_difference():
    c = R.BwdCase(1, 5, 2)
    g = torch.Generator().manual_seed(3)
    qkv, dO = torch.randn(1, 5, 3 * c.C, generator=g).double(), torch.randn(1, 5, c.C, generator=g).double()
    dq, dk, dv, lse2, delta, o = R.backward_f64(qkv, dO, c)
    grad = torch.stack([dq, dk, dv], dim=2).reshape(1, 5, 3 * c.C)

    def loss(x):
        q, k, v = R._split_heads(x, c, torch.float64)
        oo = torch.softmax((q @ k.transpose(-1, -2)) * c.scale, dim=-1) @ v
        return float((dO.view(1, 5, c.heads, 32).transpose(1, 2) * oo).sum())

    eps = 1e-6
    for idx in [(0, 0, 0), (0, 2, 17), (0, 4, 40), (0, 1, c.C + 3), (0, 3, c.C + 50), (0, 0, 2 * c.C), (0, 4, 3 * c.C - 1), (0, 2, 2 * c.C + 33)]:
        hi, lo = qkv.clone(), qkv.clone()
        hi[idx] += eps
        lo[idx] -= eps
        fd = (loss(hi) - loss(lo)) / (2 * eps)
        assert abs(fd - float(grad[idx])) <= 1e-7 * max(1.0, abs(fd)), (idx, fd, float(grad[idx]))
    assert torch.allclose(delta, (dO.view(1, 5, c.heads, 32) * o).sum(-1).transpose(1, 2), rtol=1e-12, atol=1e-12)       # sum_j P dP == sum_d dO o
    q, k, _ = R._split_heads(qkv, c, torch.float64)
    s2 = (q @ k.transpose(-1, -2)) * c.scale * R.LOG2E_F32
    assert torch.allclose(lse2, torch.log2(torch.exp2(s2).sum(-1)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_selection_inputs_are_one_hot_and_the_emulations_select_exactly(name):
    c = R.CASE_BY_NAME[name]
    q, k, v, pi = R.selection_inputs(c)
    vis = R.visible(c)
    for b in range(c.B):
        for h in range(c.heads):
            assert bool(vis[b, 0, torch.arange(c.T), pi[b, h]].all()), f"{name}: a selected key is masked"
    qq, kk, _ = R._heads_first(q, k, v, c, torch.float64)
    s = (qq @ kk.transpose(-1, -2))
    top = s.gather(-1, pi[..., None]).squeeze(-1)
    assert bool((top == 512.0 * c.D).all())
    others = s.scatter(-1, pi[..., None], float("-inf")).max(dim=-1).values
    assert bool((others <= 512.0 * (c.D - 4)).all())
    want = R.selection_expected(v, pi, c)
    for kernel in {c.route} | ({"attention_kernel"} if c.D == 32 else set()):
        got = R.emulate_forward(q, k, v, c, kernel=kernel)
        assert torch.equal(got, want), f"{name}: the {kernel} emulation does not select v row pi(i)"


@pytest.mark.parametrize("name", [c.name for c in R.BWD_CASES])
@pytest.mark.parametrize("many", [False, True])
def test_backward_selection_inputs_and_emulation(name, many):
    c = R.BWD_BY_NAME[name]
    qkv, dO, pi = R.bwd_selection_inputs(c, many)
    if not many:
        assert bool((pi.sort(dim=-1).values == torch.arange(c.T)).all()), "not a permutation"
    assert torch.equal(R.bf(qkv), qkv) and torch.equal(R.h16(qkv), qkv) and torch.equal(R.h16(dO), dO)
    dv, lse2, delta = R.bwd_selection_expected(qkv, dO, pi, c)
    assert torch.equal(R.h16(dv), dv)
    edq, edk, edv, else2, edelta = R.emulate_backward(qkv, dO, c)
    assert torch.equal(edv, dv) and torch.equal(else2, lse2) and torch.equal(edelta, delta)
    assert bool((edq == 0).all()) and bool((edk == 0).all())
    d64 = R.backward_f64(qkv, dO, c)
    assert float((d64[2] - dv.double()).abs().max()) < 1e-9 and float(d64[0].abs().max()) < 1e-9 and float(d64[1].abs().max()) < 1e-9


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_constant_v_on_the_emulations(name):
    """attention32_kernel's arithmetic returns c_d bit for bit (numerator and row sum hold the same rounded P); attention_kernel's stays within one bf16 ulp"""
    c = R.CASE_BY_NAME[name]
    for kind in R.FWD_KINDS:
        for variant in R.constant_v_variants(c, kind):
            q, k, v, cd = R.constant_v_inputs(c, kind, variant)
            assert torch.equal(R.bf(q), q) and torch.equal(R.bf(k), k)
            if variant in ("first_tile_max", "rising_max"):
                tm = R.tile_maxima(q, k, c)
                if variant == "first_tile_max":
                    assert bool((tm[..., 0:1] > tm[..., 1:]).all()), "a later tile moves a maximum"
                else:
                    assert bool((tm[..., 1:] > tm[..., :-1]).all()), "the maximum does not rise in every tile"
            dev, off, n = R.constant_v_deviation(R.emulate_forward(q, k, v, c), cd, c)
            print(f"[{name} {kind} {variant}] emulation: {off} of {n} elements differ from c_d, worst {float(dev.max()):.2f} ulp")
            if c.route == "attention32_kernel":
                assert off == 0, f"{name} {kind} {variant}: {off} of {n} elements differ from c_d"
            else:
                assert float(dev.max()) <= 1.0, f"{name} {kind}: {float(dev.max())} ulp"


def test_the_checks_tell_the_three_broken_arithmetics(monkeypatch):
    """(b) an un-rounded row sum in attention32_kernel fails constant V; (c) delta from the bf16-rounded forward output fails the peaked backward parity bound;
    (a) two swapped key slots in the V fragment order fail the selection check"""
    c = R.CASE_BY_NAME["a32_gqa"]
    q, k, v, cd = R.constant_v_inputs(c, "gauss", "plateau")
    _, off, n = R.constant_v_deviation(R.emulate_forward(q, k, v, c, denominator_from_rounded_p=False), cd, c)
    assert off > n // 100, (off, n)
    r = R.backward_reference("b1_T256_h4", "peaked")
    broken = R.backward_measures(*R.emulate_backward(r["qkv"], r["dO"], r["case"], delta_from_exponentials=False), r)
    assert broken["dq"] > 2.0 * r["emu_measures"]["dq"] and broken["dk"] > 2.0 * r["emu_measures"]["dk"], (broken, r["emu_measures"])
    step = R._pv_step

    def swapped(acc, p, x):
        if x.shape[-2] >= 2:
            x = x.clone()
            x[..., [0, 1], :] = x[..., [1, 0], :]
        return step(acc, p, x)

    monkeypatch.setattr(R, "_pv_step", swapped)
    for name in ("a32_one_tile", "gen_d32_T49", "gen_d64_causal_ragged"):
        c = R.CASE_BY_NAME[name]
        q, k, v, pi = R.selection_inputs(c)
        assert not torch.equal(R.emulate_forward(q, k, v, c), R.selection_expected(v, pi, c)), name
    cb = R.BWD_BY_NAME["b2_T100_h3"]
    qkv, dO, pi = R.bwd_selection_inputs(cb)
    assert not torch.equal(R.emulate_backward(qkv, dO, cb)[2], R.bwd_selection_expected(qkv, dO, pi, cb)[0])
