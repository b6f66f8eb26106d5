"""CPU: the dense-GEMM suite's own machinery (tests/gemm_util.py) -- the route mirror on both sides of every threshold of launch_gemm, the case list's
coverage of every reachable kernel instance and reducer, the mirror against the library's own planner (fv_op_gemm_plan: the case list at three CU counts, the
threshold shapes, the refusals, a seeded sweep), the exact class's budget, and proof that the new checks fail on broken arithmetic that the old
rel-L2 / max-abs bar lets through.  tests/test_gpu_gemm.py runs the same cases and checks on the device."""
import torch

import gemm_util as G
from gemm_util import BIAS, F16, F32, GELU, LS_RES, MUL_AUX, RES_F32, SWIGLU, SWIGLU_F16, SWIGLU_SPLIT, CASE, CASES, Case, describe, gemm_route, key, route_key

BIG = 1 << 34


def _k(**kw):
    return gemm_route(**kw)["kernel"]


# ------------------------------------------------------------------------------------------------ the mirror, both sides of every threshold (256 CUs)
def test_glds_tile_thresholds():
    t = G.glds_tile
    # 128 tiles of 256 for M <= 2048, 320 above
    assert t(2048, 4096, 128, 128, BIAS) == 256 and t(2048, 3840, 128, 128, BIAS) == 0            # 128 | 120 tiles
    assert t(4096, 5120, 128, 128, SWIGLU_F16) == 256 and t(4096, 4864, 128, 128, SWIGLU_F16) == 0   # 320 | 304 tiles (K = 128: no 128-tile rule)
    assert t(4096, 4864, 128, 128, BIAS) == 256 and t(4096, 4864, 128, 128, SWIGLU_SPLIT) == 256   # ... which binds SWIGLU_F16 alone: whole tiles have fill 1, and the
    assert t(4096, 2048, 128, 128, BIAS) == 256 and t(4096, 1792, 128, 128, BIAS) == 0            # ragged rule below takes every other epilogue from 128 tiles up (128 | 112)
    assert t(2304, 4096, 128, 128, BIAS) == 256 and t(2304, 3584, 128, 128, BIAS) == 0            # M > 2048, ragged rule: 144 | 126 tiles
    # K: a multiple of 64, at least 128
    assert t(2048, 4096, 64, 64, BIAS) == 0 and t(2048, 4096, 160, 160, BIAS) == 0 and t(2048, 4096, 192, 192, BIAS) == 256
    # ragged: fill 0.75 (16 x 8 tiles: M = 3841 is 15.004 / 16 rows full; N = 1544 is 6.03 / 7 columns)
    assert t(3848, 2048, 128, 128, F32) == 256                                                    # 16 x 8, fill 0.94
    assert t(4096, 1800, 128, 128, F32) == 256 and t(4096, 1544, 128, 128, F32) == 0              # 16 x 8 at fill 0.88 | 16 x 7 = 112 tiles
    assert t(32768, 200, 128, 128, F32) == 256 and t(32768, 184, 128, 128, F32) == 0              # 128 x 1 tiles: fill 0.78 | 0.72
    assert t(2040, 4104, 128, 128, SWIGLU_SPLIT) == 0 and t(2040, 4096, 128, 128, SWIGLU_SPLIT) == 256   # SwiGLU: ragged rows only
    assert t(2040, 4096, 128, 128, SWIGLU_F16) == 0 and t(2040, 4096, 128, 128, SWIGLU) == 0
    assert t(2048, 4096, 128, 128, SWIGLU_SPLIT, bias=True) == 0
    # the 128-tile instance: K 512 .. 1024, >= 128 tiles of 128, never fp16 operands
    assert t(1152, 1920, 512, 512, F32) == 128 and t(1152, 1920, 448, 448, F32) == 0 and t(1152, 1920, 1024, 1024, F32) == 128 and t(1152, 1920, 1088, 1088, F32) == 0
    assert t(1024, 2048, 512, 512, F32) == 128 and t(1024, 1920, 512, 512, F32) == 0              # 128 | 120 tiles
    assert t(1152, 1920, 512, 512, F32, f16=True) == 0
    # operands of 4 GiB
    assert t(1 << 20, 2048, 2048, 2048, F32) == 0 and t((1 << 20) - 256, 2048, 2048, 2048, F32) == 256


def test_register_staged_rows_and_pointwise():
    assert gemm_route(M=4096, N=2048, K=72, epi=BIAS)["grid"] == 512 and _k(M=4096, N=2048, K=72, epi=BIAS) == "gemm_kernel<128>"       # exactly 512 blocks
    assert _k(M=4088, N=2048, K=72, epi=BIAS) == "gemm_kernel<128>" and _k(M=3968, N=2048, K=72, epi=BIAS) == "gemm_kernel<64>"         # 32 x 16 = 512 | 31 x 16
    assert _k(M=384, N=96, K=96, epi=BIAS) == "pwconv_kernel<96>" and _k(M=384, N=96, K=96, lda=104, epi=BIAS) == "gemm_kernel<64>"
    assert _k(M=384, N=96, K=96, ldo=104, epi=BIAS) == "gemm_kernel<64>" and _k(M=392, N=96, K=96, epi=BIAS) == "gemm_kernel<64>"
    assert _k(M=384, N=96, K=96, epi=LS_RES) == "gemm_kernel<64>" and _k(M=384, N=96, K=96, epi=BIAS, f16=True) == "gemm_kernel<64,F16>"
    assert gemm_route(M=128 * 773, N=96, K=96, epi=BIAS)["grid"] == 768 and gemm_route(M=128 * 259, N=192, K=192, epi=BIAS)["grid"] == 256
    assert gemm_route(M=128 * 768, N=96, K=96, epi=BIAS)["grid"] == 768 and gemm_route(M=128 * 255, N=192, K=192, epi=BIAS)["grid"] == 255


def test_walks_and_asym():
    w = lambda M, N: gemm_route(M=M, N=N, K=128, epi=BIAS)      # noqa: E731
    assert w(2048, 4096)["walk"] == "column-major" and w(2304, 4096)["walk"] == "row-major"                # 8 | 9 row tiles (9 divides by neither 4 nor 2)
    assert w(3072, 6912)["walk"] == "group_m 4" and w(2560, 8192)["walk"] == "group_m 2" and w(2816, 8192)["walk"] == "row-major"     # 12 | 10 | 11 row tiles
    assert w(10240, 2048)["walk"] == "row-major" and w(10240, 2304)["walk"] == "group_m 4"                   # 8 | 9 column tiles: grouped only above 8
    assert w(8192, 2560)["kernel"] == "gemm256_kernel<8,4,ASYM>" and w(8448, 2560)["kernel"] == "gemm256_kernel<8,4>"      # ASYM: M <= 8192
    assert w(2040, 4104)["kernel"] == "gemm256_kernel<8,4>"                                                  # ... and whole row tiles
    assert G.pick_group_m(11, 4) == 0 and G.pick_group_m(12, 4) == 4 and G.pick_group_m(10, 4) == 2 and G.pick_group_m(10, 0) == 0
    # what tests/test_gpu_ops.py's ragged cases run (its docstring used to claim a grouped walk with a last group of 3)
    assert gemm_route(M=2660, N=2920, K=128, epi=F32)["walk"] == "row-major"
    ws = 8 * 1024 * 1024 * 4
    r = gemm_route(M=2660, N=2920, K=1024, epi=F32, ksplit=1, scratch=ws)
    assert r["walk"] == "row-major" and r["splits"] == 1                                                      # two ranges of partials do not fit its scratch
    r = gemm_route(M=900, N=904, K=4096, epi=F32, scratch=ws)
    assert route_key(r) == key("gemm_kernel<64>", None, True, "splitk_reduce_kernel") and r["splits"] == 5   # the few-row rule takes it before the 256-tile split-K
    r = gemm_route(M=896, N=4864, K=2048, epi=F32, ksplit=1, scratch=ws)
    assert route_key(r) == key("gemm_kernel<64>")                                                            # 532 tiles of 64 rows: no ranges; 2 x 896 x 4864 partials do not fit
    assert route_key(gemm_route(M=1152, N=896, K=2048, epi=F32, ksplit=1, scratch=ws)) == key("gemm256_kernel<8,4>", "column-major", True, "splitk_reduce_kernel")


def test_k_range_rules():
    sk = lambda **kw: gemm_route(epi=F32, scratch=BIG, **kw)      # noqa: E731
    # the few-row rule: M <= 256, or M % 256 != 0 and M <= 1024; fewer tiles than CUs; >= 4 K-tiles per range
    assert sk(M=256, N=136, K=1024)["kernel"] == "gemm_kernel<64>" and sk(M=256, N=136, K=1024)["splits"] == 4
    assert sk(M=1016, N=136, K=1024)["splits"] == 4 and sk(M=1016, N=136, K=1024)["kernel"] == "gemm_kernel<64>"      # 32 tiles: ceil(512 / 32) = 16, nkt / 4 = 4
    assert sk(M=1032, N=136, K=1024)["kernel"] != "gemm_kernel<64>" or sk(M=1032, N=136, K=1024)["splits"] == 1
    assert sk(M=512, N=1024, K=2048)["kernel"] == "gemm256_kernel<8,4,ASYM>"                                           # M % 256 == 0 above 256: not the few-row rule
    assert sk(M=77, N=136, K=448)["splits"] == 1 and sk(M=77, N=136, K=512)["splits"] == 2                              # nkt / 4: 7 / 4 = 1 | 8 / 4 = 2
    assert sk(M=256, N=16384, K=1024)["splits"] == 1 and sk(M=256, N=8064, K=1024)["splits"] == 3                       # 512 tiles >= CUs | 252 tiles
    assert gemm_route(M=77, N=136, K=1024, epi=F32, scratch=BIG, few_rows=0)["kernel"] == "gemm_kernel<64>" and \
        gemm_route(M=77, N=136, K=1024, epi=F32, scratch=BIG, few_rows=0)["splits"] == 1                                 # the training path's setting: one tile of 256, 16 K-tiles
    assert gemm_route(M=77, N=136, K=1024, epi=F32, scratch=3 * 77 * 256 * 4)["splits"] == 3                            # the scratch caps the ranges
    # bf16 epilogues: K % 64 == 0, K >= 24 tiles, tiles x 8 <= 3 CUs, >= 8 K-tiles per range
    bk = lambda **kw: gemm_route(epi=BIAS, scratch=BIG, **kw)     # noqa: E731
    assert bk(M=77, N=136, K=1536)["splits"] == 3 and bk(M=77, N=136, K=1472)["splits"] == 1 and bk(M=77, N=136, K=1544)["splits"] == 1
    assert bk(M=64 * 96, N=128, K=1536)["splits"] == 3 and bk(M=64 * 97, N=128, K=1536)["splits"] == 1                  # 96 x 8 = 768 = 3 CUs | 97
    assert gemm_route(M=77, N=136, K=1536, epi=BIAS, scratch=BIG, ksplit=1, lda=3072)["splits"] == 1
    # 256-tile split-K: K % 64, >= 16 K-tiles per range, at most 8 ranges, the cost model
    assert sk(M=512, N=1024, K=2048)["splits"] == 2 and sk(M=512, N=1024, K=1984)["splits"] == 1                        # 32 | 31 K-tiles
    assert sk(M=512, N=1024, K=8192)["splits"] == 8 and gemm_route(M=512, N=1024, K=8192, epi=F32, scratch=3 * 512 * 1024 * 4)["splits"] == 3
    assert sk(M=512, N=1024, K=65536)["splits"] == 8
    assert sk(M=1160, N=904, K=2048)["kernel"] == "gemm256_kernel<8,4>" and sk(M=1160, N=904, K=2048)["splits"] == 2
    assert sk(M=512, N=1024, K=2048, ksplit=2, lda=4096)["splits"] == 3                                                 # hi + lo8: 32 + 16 K-tiles
    assert sk(M=512, N=1024, K=2048, f16=True)["kernel"] == "gemm256_kernel<8,4,ASYM,F16>"
    # TN: up to 256 ranges
    assert gemm_route(M=520, N=264, K=2048, lda=528, ldw=280, epi=F32, tn=True, scratch=BIG)["splits"] == 2
    assert gemm_route(M=520, N=264, K=2048, lda=528, ldw=280, epi=F32, tn=True)["splits"] == 1
    assert gemm_route(M=256, N=256, K=64 * 16 * 300, lda=256, ldw=256, epi=F32, tn=True, scratch=BIG)["splits"] > 8


def test_the_tail_cut():
    t = lambda **kw: gemm_route(epi=RES_F32, ksplit=1, scratch=BIG, **kw)     # noqa: E731
    r = t(M=1024, N=17408, K=1024)
    assert isinstance(r, list) and r[0]["cols"] == (0, 16384) and r[1]["cols"] == (16384, 17408) and r[1]["splits"] == 2 and r[0]["splits"] == 1
    assert not isinstance(t(M=1024, N=16384, K=1024), list)                            # 256 tiles: exactly one round
    assert not isinstance(t(M=1024, N=16384 + 256 * 33, K=1024), list)                 # 132 tiles left: more than half a round
    assert isinstance(t(M=1024, N=16384 + 256 * 32, K=1024), list)                     # 128: exactly half
    assert not isinstance(t(M=768, N=256 * 86, K=1024), list)                          # 258 tiles, 2 left: no whole column panel of 3 row tiles
    assert not isinstance(t(M=1024, N=17408, K=960), list) and isinstance(t(M=1024, N=17408, K=1024), list)     # 30 | 32 K-tiles over both halves
    assert not isinstance(gemm_route(M=1024, N=17408, K=1024, epi=RES_F32, ksplit=1), list)                       # no scratch
    assert not isinstance(gemm_route(M=1024, N=17408, K=1024, epi=RES_F32, ksplit=1, scratch=BIG, few_rows=0), list)
    assert not isinstance(gemm_route(M=1024, N=17408, K=1024, epi=RES_F32, ksplit=1, scratch=BIG, norm=True, ldo=17408), list)
    assert not isinstance(gemm_route(M=1024, N=17408, K=1024, epi=F32, scratch=BIG, f16=True), list)
    assert not isinstance(gemm_route(M=1024, N=17408, K=1024, epi=BIAS, scratch=BIG), list)
    assert isinstance(gemm_route(M=1024, N=17408, K=1024, epi=SWIGLU_SPLIT, ksplit=1, scratch=BIG), list)        # N % 512 == 0
    assert not isinstance(gemm_route(M=1024, N=17408 + 256, K=1024, epi=SWIGLU_SPLIT, ksplit=1, scratch=BIG), list)


def test_the_fused_norm_placement():
    n = lambda **kw: gemm_route(epi=RES_F32, ksplit=1, norm=True, **kw)     # noqa: E731
    assert n(M=4096, N=896, K=2432, scratch=BIG)["reducer"] == "splitk_reduce_norm_row_kernel"             # few_rows defaults to 1: a block per row whatever the tile
    assert n(M=4096, N=896, K=2432, scratch=BIG, few_rows=0)["reducer"] == "splitk_reduce_norm_kernel"
    assert n(M=512, N=4096, K=2048, scratch=BIG)["reducer"] == "splitk_reduce_norm_row_kernel" and n(M=512, N=4352, K=2048, scratch=BIG)["reducer"] == "splitk_reduce_norm_kernel"
    assert n(M=4096, N=896, K=2432)["norm"] == "separate" and n(M=4096, N=896, K=2432, scratch=BIG)["norm"] == "fused"


# ------------------------------------------------------------------------------------------------ the mirror against the library's planner
# fv_op_gemm_plan answers with plan_gemm, the function launch_gemm runs: it makes no HIP call and reads no operand, so the comparison needs no device.
def _agree(what, **kw):
    """the mirror's route, after the library's planner has given the same one field for field (or both have refused)"""
    from fastvla_hip import _lib
    want, got = G.gemm_route(**kw), G.library_route(_lib.load_testops(), **kw)
    if G.refused(want) or G.refused(got):
        assert G.refused(want) and G.refused(got), f"{what} {kw}: plan_gemm says {describe(got)}, the mirror {describe(want)}"
    else:
        assert got == want, f"{what} {kw}: plan_gemm says {describe(got)} {got}, the mirror {describe(want)} {want}"
    return want


OTHER_CUS = (64, 304)         # with the present cases both move a threshold: asserted below


def test_the_library_plans_every_case_as_the_mirror():
    moved = {cus: 0 for cus in OTHER_CUS}
    for c in CASES:
        for epi in sorted(set(c.epis) | set(c.gauss)):
            for scratch in (c.scratch or 64 << 20, 0):
                at256 = _agree(c.name, **c.route_args(epi, G.CUS, scratch))
                for cus in OTHER_CUS:
                    moved[cus] += route_key(_agree(c.name, **c.route_args(epi, cus, scratch))) != route_key(at256)
            assert not G.refused(c.route(epi))
    assert all(moved.values()), moved


def test_the_library_refuses_what_the_mirror_refuses():
    for what, kw in G.REFUSED:
        assert G.refused(_agree(what, **kw)), what


def test_the_library_agrees_on_both_sides_of_every_threshold(monkeypatch):
    """The threshold tests above, run again with every problem they put to the mirror also put to plan_gemm (a glds_tile question as the launch without scratch)."""
    import sys
    asked, mirror_tile, busy = [], G.glds_tile, []

    def route(**kw):
        asked.append(kw)
        busy.append(1)
        try:
            return _agree("threshold", **kw)
        finally:
            busy.pop()

    def tile(M, N, K, lda, epi, f16=False, bias=False):
        if not busy:                                      # (gemm_route asks glds_tile itself)
            route(M=M, N=N, K=K, lda=lda, epi=epi, f16=f16, bias=bias)
        return mirror_tile(M, N, K, lda, epi, f16, bias)

    monkeypatch.setattr(sys.modules[__name__], "gemm_route", route)      # what the threshold tests call; _agree asks G.gemm_route
    monkeypatch.setattr(G, "glds_tile", tile)
    for test in (test_glds_tile_thresholds, test_register_staged_rows_and_pointwise, test_walks_and_asym, test_k_range_rules, test_the_tail_cut,
                 test_the_fused_norm_placement):
        test()
    assert len(asked) >= 100, len(asked)                  # (113 when this was written: the patches took hold)


SWEEP_M = (8, 64, 77, 136, 256, 320, 384, 512, 1024, 2048, 4096, 4104, 8192, 10240, 16384, 65536)
SWEEP_N = (96, 136, 144, 192, 256, 512, 896, 1024, 1152, 1536, 2048, 4864, 9728, 17920, 37888)
SWEEP_K = (72, 96, 128, 192, 360, 512, 896, 1024, 1536, 2048, 3584, 4864)


def sweep_problems(n=6000, seed=1):
    import random
    rnd = random.Random(seed)
    for _ in range(n):
        yield dict(M=rnd.choice(SWEEP_M), N=rnd.choice(SWEEP_N), K=rnd.choice(SWEEP_K), epi=rnd.choice(sorted(G.EPI_NAME)),
                   ksplit=rnd.choice((0, 1, 2)) if rnd.random() < 0.5 else 0, f16=rnd.random() < 0.15, tn=rnd.random() < 0.10,
                   scratch=rnd.choice((0, 64 << 20, 512 << 20)), few_rows=rnd.choice((0, 1)), norm=rnd.random() < 0.15, cus=rnd.choice((G.CUS,) + OTHER_CUS),
                   bias=rnd.random() < 0.5)


def test_the_library_agrees_with_the_mirror_on_a_sweep():
    """6000 seeded problems (tight strides), refusals included.  With this seed the mirror admits 3440 of them (57 %), cuts the tail off twice and reaches every
    reachable instance (the two pointwise ones twice each) and every reducer; the three conditions below keep the sweep from passing by refusing."""
    kernels, reducers, admitted, tails = {}, {}, 0, 0
    for kw in sweep_problems():
        r = _agree("sweep", **kw)
        if G.refused(r):
            continue
        admitted += 1
        tails += isinstance(r, list)
        for x in (r if isinstance(r, list) else [r]):
            kernels[x["kernel"]] = kernels.get(x["kernel"], 0) + 1
            reducers[x["reducer"]] = reducers.get(x["reducer"], 0) + 1
    print(f"[gemm plan sweep] admitted {admitted} of 6000, tail cuts {tails}, launches by kernel {kernels}, by reducer {reducers}")
    assert admitted >= 3000
    assert set(kernels) >= set(G.REACHABLE) - {"pwconv_kernel<96>", "pwconv_kernel<192>"} and not set(kernels) & set(G.UNREACHABLE)
    assert set(reducers) >= set(G.REDUCERS)


# ------------------------------------------------------------------------------------------------ the case list
def test_every_case_reaches_its_route_on_256_cus():
    for c in CASES:
        for epi in sorted(set(c.epis) | set(c.gauss)):
            r = c.route(epi)
            assert route_key(r) == c.expect, f"{c.name} {G.EPI_NAME[epi]}: expected {c.expect}, the mirror says {describe(r)}"
    c = CASE["splitk-short-scratch"]
    assert c.route(F32)["splits"] == 3 and c.route(F32, scratch=BIG)["splits"] == 8
    assert CASE["skinny-ksplit"].route(RES_F32)["splits"] == 3                       # 12 K-tiles over 3 ranges: the seam of the halves (tile 6) inside the second
    assert CASE["pw96-second-trip"].route(BIAS)["grid"] == 768 and CASE["pw192-second-trip"].route(BIAS)["grid"] == 256


def test_every_reachable_instance_and_reducer_has_a_case():
    ks, rs, ws, ns = G.covered()
    assert ks == set(G.REACHABLE), (sorted(set(G.REACHABLE) - ks), sorted(ks - set(G.REACHABLE)))
    assert rs == set(G.REDUCERS), sorted(set(G.REDUCERS) - rs)
    assert ws == set(G.WALKS) and ns == {"fused", "separate"}
    assert any(isinstance(c.route(e), list) for c in CASES for e in c.epis + c.gauss)           # the tail
    assert not (set(G.UNREACHABLE) & ks)
    # ragged edges under a grouped walk, K ranges on ragged 256-tiles, the reducers' bf16 epilogues: each by name
    assert CASE["ragged-group4"].route(F32)["walk"] == "group_m 4" and CASE["ragged-group4"].M % 256 and CASE["ragged-group4"].N % 256
    assert CASE["splitk-ragged"].route(F32)["kernel"] == "gemm256_kernel<8,4>" and CASE["splitk-ragged"].route(F32)["splits"] > 1
    assert {BIAS, GELU, LS_RES} <= set(CASE["skinny-bf16"].epis + CASE["skinny-bf16"].gauss)


def test_every_instance_runs_every_epilogue_it_admits():
    """Each instance compiles its own epilogue and guarded store loop: the case list runs, through every kernel in one pass and through every reducer, exactly
    the epilogues gemm_util.EPILOGUES / REDUCER_EPILOGUES name -- all that launch_gemm admits there and an op-level entry point can express.  What is left out is
    listed in gemm_util.OMITTED with its reason.  The linear ones are in the exact class, the nonlinear ones in the Gaussian class only."""
    assert set(G.EPILOGUES) == set(G.REACHABLE) and set(G.REDUCER_EPILOGUES) == set(G.REDUCERS)
    cov = G.covered_epilogues()
    name = lambda es: sorted(G.EPI_NAME[e] for e in es)      # noqa: E731
    for k, want in G.EPILOGUES.items():
        assert cov.get(k, set()) == want, f"{k}: missing {name(want - cov.get(k, set()))}, unexpected {name(cov.get(k, set()) - want)}"
    assert G.covered_reducer_epilogues() == G.REDUCER_EPILOGUES
    linear = {BIAS, LS_RES, F32, RES_F32, F16, MUL_AUX}
    for c in CASES:
        assert set(c.epis) <= linear and not (set(c.gauss) - linear - {GELU, SWIGLU, SWIGLU_SPLIT, SWIGLU_F16})
    exact = {}
    for c in CASES:
        for epi in c.epis:
            r = c.route(epi)
            if not isinstance(r, list) and r["splits"] == 1:
                exact.setdefault(r["kernel"], set()).add(epi)
    for k, want in G.EPILOGUES.items():
        assert exact.get(k, set()) == want & linear, f"{k}: linear epilogues outside the exact class: {name((want & linear) - exact.get(k, set()))}"
    # the admitted epilogues are what the mirror says the dispatcher takes: fp16 operands refuse GELU, LS_RES, SWIGLU; ksplit refuses the fp16-output ones
    for epi in (GELU, LS_RES, SWIGLU):
        assert G.refused(gemm_route(M=77, N=144, K=72, epi=epi, f16=True))
    for epi in (F16, MUL_AUX):
        assert G.refused(gemm_route(M=77, N=136, K=128, lda=256, epi=epi, ksplit=2)) and G.refused(gemm_route(M=77, N=136, K=128, epi=epi, ksplit=1))
    assert G.glds_tile(2048, 4096, 128, 128, SWIGLU) == 0                          # plain SWIGLU never reaches a 256-tile instance
    assert all(len(why) > 20 for why in G.OMITTED.values())


def test_unreachable_instances_are_unreachable():
    """gemm256_kernel<4,2,F16>: glds_instance names it (a 128-tile with fp16 operands), but gemm_glds_tile never returns 128 for fp16 operands in the product
    build.  Sweep the shapes the 128-tile rule admits."""
    for M in (1024, 1152, 4096):
        for N in (1920, 2048, 896 * 4):
            for K in (512, 768, 1024):
                for epi in (F32, RES_F32, BIAS, F16, MUL_AUX, SWIGLU_SPLIT, SWIGLU_F16):
                    r = gemm_route(M=M, N=N, K=K, epi=epi, f16=True)
                    assert G.refused(r) or r["kernel"] not in G.UNREACHABLE, (M, N, K, epi, describe(r))
                    assert G.glds_tile(M, N, K, K, epi, f16=True) != 128


def test_refusals():
    for what, kw in G.REFUSED:
        assert G.refused(gemm_route(**kw)), what


def test_exact_class_budget():
    """max|A| max|W| K_total + |bias| + |res| in units of q stays below 2^22 (2^21 under LS_RES) for every case and epilogue, and the generated values keep to
    their ranges"""
    for c in CASES:
        for epi in c.epis:
            total, limit = G.exact_budget(c, epi)
            assert total <= limit <= 2.0 ** 22, (c.name, epi, total, limit)
            a, w, _, _, _, _ = G.exact_ranges(c, epi)
            assert a >= 1 and w >= 1
    for name in ("g64", "g64-ksplit", "g64-lo8", "skinny-bf16", "tn"):
        c = CASE[name]
        for epi in c.epis:
            p = G.exact_problem(c, epi)
            a, w, (b_lo, b_hi), rmax, q, limit = G.exact_ranges(c, epi)
            assert float(p.Wval.abs().max()) <= w and float(p.Aval.abs().max()) < a + 1
            pre, ab = G.reference(p)
            worst = ab + (p.bias.double().abs() if p.bias is not None else 0.0)
            assert float(worst.max()) < limit
            assert bool(((pre / q) == (pre / q).round()).all())
            if c.ksplit == 2:
                assert torch.equal(p.W8val, p.Wval)


def test_exact_class_outputs_need_rounding_and_hit_ties():
    for name, epi in (("g64", BIAS), ("g64", LS_RES), ("g64-f16", F16), ("g64-f16", MUL_AUX), ("g64-ksplit", BIAS), ("skinny-bf16", BIAS)):
        p = G.exact_problem(CASE[name], epi)
        need, tie = G.rounding_census(G.exact_expected(p), G.out_dtype(epi))
        print(f"[gemm exact] {name} {G.EPI_NAME[epi]}: {need:.2f} of the outputs need rounding, {tie:.3f} are ties")
        # (a split operand's sums are multiples of 2^-8: a tie needs all eight fraction bits right, one output in a thousand)
        assert need >= 0.5 and tie >= (0.0003 if CASE[name].ksplit else 0.01), (name, epi, need, tie)


def test_selection_class_covers_every_k():
    for name in ("g64", "g64-ksplit", "g64-lo8", "skinny-bf16", "tn", "asym-colmajor-ksplit"):
        c = CASE[name]
        seen = torch.zeros(c.ktotal, dtype=torch.bool)
        for launch in range(G.selection_launches(c)):
            p, pi = G.selection_problem(c, c.epis[0], launch)
            seen[pi[pi >= 0]] = True
            assert bool((pi[torch.arange(c.M) % 11 == 7] == -1).all())
        assert bool(seen.all()), name
    # the lo8 form's weights: e4m3(64 W) is W itself (nothing saturates), and all 128 slots of an fp8 step differ
    W = G.selection_weights(300, 1600, lo8=True)
    assert torch.equal(G.e4m3(W * 64.0).double() / 64.0, W) and torch.equal(W, W.bfloat16().double()) and float(W.abs().min()) > 0
    for t in range(0, 1600 - 128, 64):
        assert all(len(set(W[n, t:t + 128].tolist())) == 128 for n in (0, 1, 150, 299))
    p, _ = G.selection_problem(CASE["g64-lo8"], F32, 0)
    assert torch.equal(p.W8val, p.Wval)
    W = G.selection_weights(300, 1600)
    assert float(W.abs().max()) <= 254 and torch.equal(W, W.bfloat16().double()) and torch.equal(W, W.half().double())
    for t in range(0, 1600 - 64, 64):
        assert all(len(set(W[n, t:t + 64].tolist())) == 64 for n in (0, 1, 150, 299))


def test_silu_emulation_error():
    x = torch.linspace(-G.SILU_RANGE, G.SILU_RANGE, 2_000_001, dtype=torch.float64).float()
    e, r = G.silu_emulated(x).double(), G.silu64(x.double())
    m = r != 0
    worst = float(((e - r).abs() / r.abs())[m].max())
    print(f"[gemm silu] float32 emulation of silu_f against float64 over |x| <= {G.SILU_RANGE}: worst relative error {worst:.3e} (SILU_ERR {G.SILU_ERR:.1e})")
    assert worst <= G.SILU_ERR
    assert G.norm_rel_bound(896) <= 2.0 ** -16 and G.norm_rel_bound(4096) <= 2.0 ** -16


# ------------------------------------------------------------------------------------------------ the checks must be able to fail
def _check_close_passes(got, ref, f32):
    """tests/gpu_util.py check_close with the bars tests/test_gpu_ops.py uses (gpu_util itself imports the device library): True = passes"""
    got, ref = got.float(), ref.float()
    if not bool(torch.isfinite(got).all()):
        return False
    rel = float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))
    m = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    return rel <= (2e-5 if f32 else 4e-3) and m <= (2e-5 if f32 else 2e-2)


def _fails(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


SMALL = Case("small", 77, 136, 200, [BIAS, LS_RES, F32, RES_F32], None, gauss=[BIAS, GELU, LS_RES, F32], ksplit=1)      # 3.125 K-tiles per half
SMALL_SW = Case("small-swiglu", 77, 144, 200, [], None, gauss=[SWIGLU, SWIGLU_SPLIT], ksplit=1)


def _exact(p, **defect):
    c, epi = p.c, p.epi
    got = G.emulate(p, **defect)
    assert bool(torch.isnan(got[:, c.ncols(epi):].float()).all()), "pad columns written"
    G.check_bits(got[:, :c.ncols(epi)], G.exact_expected(p), f"{c.name} {G.EPI_NAME[epi]}")


def _select(c, epi, **defect):
    for launch in range(G.selection_launches(c)):
        p, pi = G.selection_problem(c, epi, launch)
        G.check_bits(G.emulate(p, **defect)[:, :c.N], G.selection_expected(p, pi), f"{c.name} selection launch {launch}")


def _gauss(p, **defect):
    c, epi = p.c, p.epi
    splits = defect.get("splits", 1)
    got = G.emulate(p, **defect)
    I = c.N // 2
    out = (got[:, :I], got[:, I:2 * I]) if epi == SWIGLU_SPLIT else got[:, :c.ncols(epi)]
    return G.gauss_check(p, out, splits, what=f"{c.name} {G.EPI_NAME[epi]} (emulation)")


def _gauss_ref(p):
    """the float64 reference the old tests compare with, in the output's layout"""
    pre, _ = G.reference(p)
    v = pre + (p.bias.double() if p.bias is not None else 0.0)
    if p.epi == LS_RES:
        v = p.res[:, :p.c.N].double() + p.scale.double() * v
    return v


def test_the_clean_emulation_passes_every_check():
    """float32 sums, one rounding: exact and selection classes bit for bit, and inside every Gaussian bound -- with one pass and with K ranges -- so the bounds are
    met by the reference arithmetic alone"""
    for epi in SMALL.epis:
        _exact(G.exact_problem(SMALL, epi))
        _exact(G.exact_problem(SMALL, epi), splits=3)
    _select(SMALL, F32)
    _select(SMALL, BIAS, splits=3)
    worst = 0.0
    for c in (SMALL, SMALL_SW):
        for epi in c.gauss:
            for splits in (1, 3):
                worst = max(worst, _gauss(G.gauss_problem(c, epi), splits=splits))
    assert 0.05 < worst <= 1.0           # and the bounds are not slack by orders of magnitude


def test_the_checks_tell_the_broken_arithmetics():
    """Each defect fails a new check; whether tests/gpu_util.py's check_close (rel-L2 <= 4e-3 and max-abs <= 2e-2 of max|ref| for bf16 outputs, 2e-5 for fp32) lets
    it pass on the suite's Gaussian data is asserted next to it.

      an output truncated to bf16                     exact class (bits), Gaussian bound (the half-ulp term)        check_close passes
      LS_RES, scaled product rounded before the add   exact class (bits)                                            check_close passes
      two k-slots swapped inside one 32-deep step     selection class, exact class                                  check_close fails (2 of 200 products wrong: 1e-1)
      the lo half's last K-tile dropped               selection class, exact class                                  check_close passes (bf16 output)
      one edge row written one row late               coverage (a NaN row), exact class                             check_close fails (non-finite output)"""
    pg = G.gauss_problem(SMALL, BIAS)
    # truncation
    assert _fails(_exact, G.exact_problem(SMALL, BIAS), truncate=True)
    assert _fails(_gauss, pg, truncate=True)
    assert _check_close_passes(G.emulate(pg, truncate=True)[:, :SMALL.N], _gauss_ref(pg), False)
    # LS_RES rounded twice
    pl = G.gauss_problem(SMALL, LS_RES)
    assert _fails(_exact, G.exact_problem(SMALL, LS_RES), double_round=True)
    assert _check_close_passes(G.emulate(pl, double_round=True)[:, :SMALL.N], _gauss_ref(pl), False)
    # k-slots 5 and 19 of the first 32-deep step
    assert _fails(_select, SMALL, F32, swap_k=(5, 19)) and _fails(_exact, G.exact_problem(SMALL, F32), swap_k=(5, 19))
    assert not _check_close_passes(G.emulate(pg, swap_k=(5, 19))[:, :SMALL.N], _gauss_ref(pg), False)
    # the lo half's last K-tile
    assert _fails(_select, SMALL, F32, drop_lo_tail=True) and _fails(_exact, G.exact_problem(SMALL, F32), drop_lo_tail=True)
    assert _check_close_passes(G.emulate(pg, drop_lo_tail=True)[:, :SMALL.N], _gauss_ref(pg), False)
    # the last row of the first 64-row tile, one row late
    got = G.emulate(G.exact_problem(SMALL, F32), late_row=63)
    assert bool(torch.isnan(got[:, :SMALL.N]).any())                                    # the coverage check of every GPU launch: no NaN left inside M x N
    assert _fails(_exact, G.exact_problem(SMALL, F32), late_row=63)
    assert not _check_close_passes(G.emulate(pg, late_row=63)[:, :SMALL.N], _gauss_ref(pg), False)
