"""CPU-only helpers of the dense-GEMM suites (tests/test_gemm_reference_host.py, tests/test_gpu_gemm.py): a mirror of launch_gemm's dispatch for the product
build (csrc/gemm_bf16.hip: plan_gemm, i.e. check_gemm, tail_cut, route_gemm and their helpers gemm_glds_tile, set_walk, k_ranges, few_row_ranges, set_ranges --
every FASTVLA_* switch of its Tuning is at its default there), library_route, which asks the library's own plan_gemm through fv_op_gemm_plan so that the two can
be compared field for field, the case list both files share, the three input classes (exact, selection, Gaussian), their checks, and float32 / bf16 emulations of a small
GEMM with defects to plant."""
import math

import torch

from dw_fwd_util import GELU_ERR, GELU_SLOPE, bf16_half_ulp, bf16_round, bf16_truncate, gelu_erf, gelu2_n_emulated, gen

BIAS, GELU, LS_RES, RES_F32, SWIGLU, F32, SWIGLU_SPLIT, SWIGLU_F16, GELU_GRAD, MUL_AUX, F16, MUL_GELUP = 0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12
EPI_NAME = {BIAS: "BIAS", GELU: "BIAS_GELU", LS_RES: "LS_RES", RES_F32: "RES_F32", SWIGLU: "SWIGLU", F32: "F32", SWIGLU_SPLIT: "SWIGLU_SPLIT",
            SWIGLU_F16: "SWIGLU_F16", GELU_GRAD: "GELU_GRAD", MUL_AUX: "MUL_AUX", F16: "F16", MUL_GELUP: "MUL_GELUP"}
F32_EPIS, F16_OUT_EPIS = (RES_F32, F32), (GELU_GRAD, MUL_AUX, MUL_GELUP, F16)
BN, BK = 128, 64               # the register-staged kernel's column tile and every kernel's K-tile
CUS = 256                      # the MI355X; the GPU file asks the device


# ------------------------------------------------------------------------------------------------ the route mirror
def pick_group_m(tiles_m_total, want):
    """set_walk's group height"""
    if want >= 4 and tiles_m_total % 4 == 0:
        return 4
    if want >= 2 and tiles_m_total % 2 == 0:
        return 2
    return 0


def glds_tile(M, N, K, lda, epi, f16=False, bias=False):
    """gemm_glds_tile: 0 (the register-staged kernel), 256 or 128"""
    if K % 64 or K < 128:
        return 0
    if M * lda * 2 >= 1 << 32 or N * K * 2 >= 1 << 32:
        return 0
    f32, f16_epi = epi in F32_EPIS, epi in F16_OUT_EPIS
    if epi not in (BIAS, GELU, LS_RES, SWIGLU_SPLIT, SWIGLU_F16) and not f32 and not f16_epi:
        return 0
    if epi in (SWIGLU_SPLIT, SWIGLU_F16) and bias:
        return 0
    if M % 256 == 0 and N % 256 == 0 and (M // 256) * (N // 256) >= (128 if M <= 2048 else 320):
        return 256
    bf16_epi = epi in (BIAS, GELU, LS_RES) or f16_epi
    if ((f32 or bf16_epi) and N % 8 == 0) or (epi == SWIGLU_SPLIT and N % 256 == 0):
        tm, tn = (M + 255) // 256, (N + 255) // 256
        fill = float(M) * N / (float(tm) * tn * 65536.0)
        if tm * tn >= 128 and fill >= 0.75:
            return 256
    if f16:
        return 0
    if M % 128 == 0 and N % 128 == 0 and (M // 128) * (N // 128) >= 128 and 512 <= K <= 1024:
        return 128
    return 0


def _walk(tmr, tn, cm_max=8, want=4):
    """(tiles_m, group_m, name) of the 256-tile kernels' tile walk"""
    tiles_m = tmr if tmr <= cm_max else 0
    group_m = pick_group_m(tmr, want) if (not tiles_m and tn > 8) else 0
    return tiles_m, group_m, "column-major" if tiles_m else (f"group_m {group_m}" if group_m else "row-major")


def _g256_name(tile, asym=False, f16=False, lo8=False, tn=False):
    flags = [n for n, on in (("ASYM", asym), ("F16", f16), ("LO8", lo8), ("TN", tn)) if on]
    return "gemm256_kernel<%s>" % ",".join(["8,4" if tile == 256 else "4,2"] + flags)


def _staged_name(bm, f16=False, lo8=False):
    return "gemm_kernel<%s>" % ",".join([str(bm)] + (["F16"] if f16 else []) + (["LO8"] if lo8 else []))


def _reducer(epi, norm, few_rows_form, few_rows, N, lo8):
    """set_ranges: (kernel, the RMSNorm went with it)"""
    if epi == SWIGLU_SPLIT:
        return "splitk_reduce_swiglu_kernel", False
    if epi in (BIAS, GELU, LS_RES):
        return "splitk_reduce_bf16_kernel", False
    if norm and (few_rows_form or few_rows) and N <= 4096 and not lo8:
        return "splitk_reduce_norm_row_kernel", True
    if norm:
        return "splitk_reduce_norm_kernel", True
    return "splitk_reduce_kernel", False


def _ranges_256(tiles, nkt, M, tn, scratch, cus, max_ranges, min_kt=16):
    """the cost model both 256-tile K-range forms share: rounds of `cus` units, each 1 / s of a tile's K loop, plus the partial sums' trip through memory"""
    tile_us = float(nkt) * 64.0 * 131072.0 / 1.0e6 / 4.0
    part_us = 2.0 * float(M) * (tn * 256) * 4.0 / 4.0e6
    best, splits = 1e30, 1
    for s in range(1, max_ranges + 1):
        if s > 1 and (nkt // s < min_kt or s * M * (tn * 256) * 4 > scratch):
            break
        rounds = (tiles * s + cus - 1) // cus
        t = float(rounds) * tile_us / s + (s * part_us if s > 1 else 0.0)
        if t < best * 0.97:
            best, splits = t, s
    return splits


def _route(kernel, tile, M, N, splits=1, npad=0, grid=0, reducer=None, walk=None, tiles_m=0, group_m=0, norm=None, cols=None):
    return {"kernel": kernel, "tile": tile, "walk": walk, "tiles_m": tiles_m, "group_m": group_m, "splits": splits, "npad": npad, "grid": grid,
            "reducer": reducer, "norm": norm, "cols": cols}


def refused(r):
    return isinstance(r, dict) and "refused" in r


def _strides(M, N, K, lda, ldo, ldr, ldw, epi, ksplit, tn):
    """the row strides a call leaves out: tight ones"""
    ncols = N // 2 if epi in (SWIGLU, SWIGLU_F16) else N
    return (lda if lda is not None else (M if tn else (2 * K if ksplit else K)), ldo if ldo is not None else ncols, ldr if ldr is not None else N,
            ldw if ldw is not None else (N if tn else 0))


def library_route(L, M, N, K, lda=None, ldo=None, epi=BIAS, ksplit=0, f16=False, tn=False, bias=False, scratch=0, few_rows=1, norm=False, cus=CUS, ldw=None,
                  ldr=None, res=True, scale=True, stash=False):
    """gemm_route's arguments, answered by the library itself: fv_op_gemm_plan (plan_gemm, what launch_gemm runs) in gemm_route's form.  L: the loaded test-ops
    library.  The weights' fp8 copy is present whenever ksplit == 2."""
    from fastvla_hip._lib import GemmPlanLaunch
    lda, ldo, ldr, ldw = _strides(M, N, K, lda, ldo, ldr, ldw, epi, ksplit, tn)
    out = (GemmPlanLaunch * 2)()
    n = L.fv_op_gemm_plan(M, N, K, lda, ldw, ldo, ldr, epi, ksplit, int(f16), int(tn), few_rows, cus, scratch, int(bool(bias)), int(bool(scale)), int(bool(res)),
                          int(bool(stash)), int(bool(norm)), int(ksplit == 2), out)
    if n <= 0:
        return {"refused": (L.fv_last_error(None) or b"?").decode()}
    routes = []
    for x in out[:n]:
        kernel = x.kernel.decode()
        walk = None if not kernel.startswith("gemm256") else "column-major" if x.tiles_m else f"group_m {x.group_m}" if x.group_m else "row-major"
        routes.append(_route(kernel, x.tile, M, N, x.splits, x.npad, x.grid, x.reducer.decode() or None, walk, x.tiles_m, x.group_m,
                             {0: None, 1: "fused", 2: "separate"}[x.norm], (x.c0, x.c1) if n == 2 else None))
    return routes if n == 2 else routes[0]


def gemm_route(M, N, K, lda=None, ldo=None, epi=BIAS, ksplit=0, f16=False, tn=False, bias=False, scratch=0, few_rows=1, norm=False, cus=CUS, ldw=None,
               ldr=None, res=True, scale=True, stash=False, no_tail=False, _cols=None):
    """What launch_gemm does with the problem in the product build: a route (dict), a LIST of two routes where the tail is cut off as a K-range problem of its
    own, or {"refused": why}.  scratch = the scratch buffer's bytes (0: none).  res / scale / stash: whether the caller hands the pointer in.  Pointer
    alignment is the one refusal this mirror cannot see."""
    f32out = epi in F32_EPIS
    swiglu = epi in (SWIGLU, SWIGLU_SPLIT, SWIGLU_F16)
    ncols = N // 2 if epi in (SWIGLU, SWIGLU_F16) else N
    lda, ldo, ldr, ldw = _strides(M, N, K, lda, ldo, ldr, ldw, epi, ksplit, tn)
    if norm and (not f32out or ldo != N or N % 8):
        return {"refused": "fused norm needs an fp32 epilogue, ldo == N and N % 8 == 0"}
    if M <= 0 or N <= 0 or K <= 0:
        return {"refused": "empty shape"}
    if tn:
        if not f32out or ksplit or norm or stash:
            return {"refused": "TN: fp32 epilogues only, no ksplit / fused norm / stash"}
        if K % 64 or M % 8 or N % 8 or lda % 8 or ldw % 8 or lda < M or ldw < N:
            return {"refused": "TN: K % 64, M % 8, N % 8, lda >= M, ldw >= N"}
        if ldo < N or ldo % 4 or (epi == RES_F32 and (not res or ldr % 4 or ldr < N)):
            return {"refused": "TN: bad ldo / residual"}
        if K * lda * 2 >= 1 << 31 or K * ldw * 2 >= 1 << 31:
            return {"refused": "TN: operands of 2 GiB or more"}
        tmr, tnn, nkt = (M + 255) // 256, (N + 255) // 256, K // 64
        splits = _ranges_256(tmr * tnn, nkt, M, tnn, scratch, cus, 256) if scratch else 1
        tiles_m, group_m, walk = _walk(tmr, tnn)
        nwg, slots = tmr * tnn * splits, cus // 8 * 8
        return _route(_g256_name(256, f16=f16, tn=True), 256, M, N, splits, tnn * 256, min(nwg, slots), "splitk_reduce_kernel" if splits > 1 else None,
                      walk, tiles_m, group_m)
    if K % 8 or lda % 8 or N % 8:
        return {"refused": "K, lda, N must be multiples of 8"}
    if lda < K:
        return {"refused": "lda < K"}
    if epi < BIAS or epi > MUL_GELUP or epi == 6:
        return {"refused": "bad epilogue"}
    if epi in F16_OUT_EPIS and ksplit:
        return {"refused": "the fp16-output epilogues take no ksplit"}
    if epi == GELU_GRAD and not stash:
        return {"refused": "GELU_GRAD needs a stash"}
    if epi in (MUL_AUX, MUL_GELUP) and (not res or ldr % 8 or ldr < N):
        return {"refused": "MUL_AUX / MUL_GELUP need the fp16 factor in res"}
    if f16 and ksplit:
        return {"refused": "fp16 operands are a single pass"}
    if f16 and epi in (GELU, LS_RES, SWIGLU):
        return {"refused": "fp16 operands go with the BIAS / F32 / RES_F32 / SWIGLU_SPLIT / SWIGLU_F16 epilogues"}
    if swiglu and N % 16:
        return {"refused": "SwiGLU needs N % 16 == 0"}
    if ldo < ncols or ldo % (4 if f32out else 8):
        return {"refused": "bad ldo"}
    if epi == LS_RES and (not res or not scale or ldr % 8 or ldr < N):
        return {"refused": "LS_RES needs res/scale"}
    if epi == RES_F32 and (not res or ldr % 4 or ldr < N):
        return {"refused": "RES_F32 needs res"}
    if ksplit == 2:
        if K % 128 or lda * 2 < 3 * K:
            return {"refused": "the hi + lo8 form needs K % 128 == 0 and lda >= 1.5 K"}
    elif ksplit and lda < 2 * K:
        return {"refused": "ksplit needs lda >= 2K"}
    asym = M <= 8192 and M % 256 == 0
    gt = glds_tile(M, N, K, lda, epi, f16, bias)
    sub = dict(lda=lda, ldo=ldo, epi=epi, ksplit=ksplit, f16=f16, bias=bias, scratch=scratch, few_rows=few_rows, cus=cus, ldr=ldr, res=res, scale=scale)
    # the tail
    if (not no_tail and few_rows and scratch and not norm and not stash and not f16 and ksplit != 2 and M % 256 == 0 and N % 256 == 0 and K % 64 == 0
            and (f32out or (epi == SWIGLU_SPLIT and N % 512 == 0)) and gt == 256):
        tmr, tnn = M // 256, N // 256
        tiles, nkt = tmr * tnn, (2 if ksplit else 1) * (K // 64)
        rem = tiles % cus
        if tiles > cus and rem > 0 and 2 * rem <= cus and rem % tmr == 0 and nkt >= 32:
            n0 = (tnn - rem // tmr) * 256
            return [gemm_route(M, n0, K, no_tail=True, _cols=(0, n0), **sub), gemm_route(M, N - n0, K, no_tail=True, _cols=(n0, N), **sub)]
    swiglu_sk = epi == SWIGLU_SPLIT and not stash and N % 16 == 0 and ksplit != 2 and not f16
    # few rows: 64-row tiles of the register-staged kernel cut along K, fp32 and SwiGLU-split epilogues
    if few_rows and scratch and (f32out or swiglu_sk) and (M <= 256 or (M % 256 != 0 and M <= 1024)) and N % 8 == 0 and ksplit != 2 and not f16:
        tnn = (N + BN - 1) // BN
        tiles, nkt, npad = ((M + 63) // 64) * tnn, (2 if ksplit else 1) * ((K + BK - 1) // BK), tnn * BN
        splits = (2 * cus + tiles - 1) // tiles if tiles < cus else 1
        splits = min(splits, nkt // 4)
        while splits > 1 and splits * M * npad * 4 > scratch:
            splits -= 1
        if splits > 1:
            red, fused = _reducer(epi, norm, True, few_rows, N, 0)
            return _route(_staged_name(64), 64, M, N, splits, npad, tiles * splits, red, norm=("fused" if fused else "separate") if norm else None, cols=_cols)
    # few 64-row tiles, long K, bf16 epilogues
    if few_rows and scratch and epi in (BIAS, GELU, LS_RES) and not ksplit and not f16 and N % 8 == 0 and K % BK == 0 and K >= 24 * BK:
        tnn = (N + BN - 1) // BN
        tiles, nkt, npad = ((M + 63) // 64) * tnn, K // BK, tnn * BN
        splits = (2 * cus + tiles - 1) // tiles if tiles * 8 <= cus * 3 else 1
        splits = min(splits, nkt // 8)
        while splits > 1 and splits * M * npad * 4 > scratch:
            splits -= 1
        if splits > 1:
            return _route(_staged_name(64), 64, M, N, splits, npad, tiles * splits, "splitk_reduce_bf16_kernel", cols=_cols)
    # 256-tile split-K
    if (scratch and (f32out or (swiglu_sk and M % 256 == 0 and N % 256 == 0)) and (M % 256 == 0 or N % 8 == 0) and K % 64 == 0 and N % 4 == 0
            and M * lda * 2 < 1 << 32 and N * K * 2 < 1 << 32):
        tmr, tnn = (M + 255) // 256, (N + 255) // 256
        tiles = tmr * tnn
        nkt = K // 64 + K // 128 if ksplit == 2 else (2 if ksplit else 1) * (K // 64)
        splits = _ranges_256(tiles, nkt, M, tnn, scratch, cus, 8)
        if splits > 1:
            tiles_m, group_m, walk = _walk(tmr, tnn)
            nwg = tiles * splits
            kern = _g256_name(256, lo8=True) if ksplit == 2 else _g256_name(256, asym=asym, f16=f16)
            red, fused = _reducer(epi, norm, False, few_rows, N, ksplit == 2)
            return _route(kern, 256, M, N, splits, tnn * 256, nwg if nwg < cus else cus // 8 * 8, red, walk, tiles_m, group_m,
                          ("fused" if fused else "separate") if norm else None, _cols)
    nm = "separate" if norm else None
    if not ksplit and not f16 and N == K and K in (96, 192) and lda == K and ldo == N and M % 128 == 0 and epi in (BIAS, GELU):
        tiles = M // 128
        return _route(f"pwconv_kernel<{K}>", 128, M, N, grid=min(tiles, 3 * cus if K == 96 else cus), norm=nm, cols=_cols)
    if gt:
        tmr, tnn = (M + gt - 1) // gt, (N + gt - 1) // gt
        tiles_m, group_m, walk = _walk(tmr, tnn)
        slots = (2 * cus if gt == 128 else cus) // 8 * 8
        if ksplit == 2:
            kern = _g256_name(gt, lo8=True)
        elif gt == 256:
            kern = _g256_name(256, asym=asym, f16=f16)
        else:
            kern = _g256_name(128, f16=f16)
        return _route(kern, gt, M, N, grid=min(tmr * tnn, slots), walk=walk, tiles_m=tiles_m, group_m=group_m, norm=nm, cols=_cols)
    tnn = (N + BN - 1) // BN
    blocks128 = ((M + 127) // 128) * tnn
    bm = 128 if blocks128 >= 512 else 64
    return _route(_staged_name(bm, f16, ksplit == 2), bm, M, N, grid=blocks128 if bm == 128 else ((M + 63) // 64) * tnn, norm=nm, cols=_cols)


def route_key(r):
    """what a case pins: kernel, walk, whether K ranges are used, the reducer, where the RMSNorm runs"""
    if isinstance(r, list):
        return tuple(route_key(x) for x in r)
    if refused(r):
        return ("refused",)
    return (r["kernel"], r["walk"], r["splits"] > 1, r["reducer"], r["norm"])


def describe(r):
    if isinstance(r, list):
        return " + ".join(f"[columns {x['cols'][0]}..{x['cols'][1]}: {describe(x)}]" for x in r)
    if refused(r):
        return "refused: " + r["refused"]
    s = f"{r['kernel']} grid {r['grid']}"
    if r["walk"]:
        s += f", {r['walk']} walk"
    if r["splits"] > 1:
        s += f", {r['splits']} K ranges (npad {r['npad']}) -> {r['reducer']}"
    if r["norm"]:
        s += f", RMSNorm {r['norm']}"
    return s


# every kernel instance launch_gemm can launch in the product build, and the second-pass kernels
REACHABLE = ["gemm_kernel<64>", "gemm_kernel<64,F16>", "gemm_kernel<64,LO8>", "gemm_kernel<128>", "gemm_kernel<128,F16>", "gemm_kernel<128,LO8>",
             "gemm256_kernel<8,4>", "gemm256_kernel<8,4,ASYM>", "gemm256_kernel<8,4,F16>", "gemm256_kernel<8,4,ASYM,F16>", "gemm256_kernel<8,4,LO8>",
             "gemm256_kernel<4,2>", "gemm256_kernel<4,2,LO8>", "gemm256_kernel<8,4,TN>", "gemm256_kernel<8,4,F16,TN>", "pwconv_kernel<96>", "pwconv_kernel<192>"]
REDUCERS = ["splitk_reduce_kernel", "splitk_reduce_norm_kernel", "splitk_reduce_norm_row_kernel", "splitk_reduce_bf16_kernel", "splitk_reduce_swiglu_kernel"]
WALKS = ["column-major", "row-major", "group_m 4", "group_m 2"]
# compiled (gemm_bf16.hip's instance table names them) but not reachable in the product build, and why
UNREACHABLE = {
    "gemm256_kernel<4,2,F16>": "gemm_glds_tile returns 0 for fp16 operands before its 128-tile rule; FASTVLA_F16_TILE128, which returns 128 earlier, is a tools-build "
                               "switch (fv_ab_env is a constant nullptr in the product build)",
}
# reachable in the library but not through any fv_op_* entry point: no op-level case can exist
NO_ENTRY_POINT = {
    "GELU_GRAD epilogue": "needs GemmArgs::stash; fv_op_gemm_f16 passes none, so the launch is refused (the tower-backward suites cover it end to end)",
    "SWIGLU_SPLIT / SWIGLU_F16 with a stash": "no op-level entry point hands a stash in",
    "splitk_reduce_norm_kernel, lo8 form": "fv_op_gemm_lo8 takes no norm_w",
}


# ------------------------------------------------------------------------------------------------ the cases both files share
def key(kernel, walk=None, ranged=False, reducer=None, norm=None):
    return (kernel, walk, ranged, reducer, norm)


class Case:
    """One problem and the route it is there for.  epis: the epilogues of the exact class (linear ones); gauss: those of the Gaussian class.  scratch: bytes of
    split-K scratch (0: none).  tight: lda == K and ldo == N (the pointwise kernel asks for it); every other case has 8 pad columns on lda, ldo and ldr."""

    def __init__(self, name, M, N, K, epis, expect, *, gauss=(), ksplit=0, f16=False, tn=False, tight=False, pad=8, scratch=0, few_rows=1, norm=False):
        self.name, self.M, self.N, self.K, self.epis, self.expect, self.gauss = name, M, N, K, tuple(epis), expect, tuple(gauss)
        self.ksplit, self.f16, self.tn, self.tight, self.scratch, self.few_rows, self.norm = ksplit, f16, tn, tight, scratch, few_rows, norm
        self.pad = 0 if tight or norm else pad
        self.kstore = M if tn else (2 * K if ksplit else K)                       # elements of a stored A row that hold data (lo8: K bf16 + K bytes, in a 2K-wide row)
        self.lda = self.kstore + (0 if tight else pad)
        self.ldw = N + 16 if tn else K
        self.ktotal = 2 * K if ksplit else K

    def ncols(self, epi):
        return self.N // 2 if epi in (SWIGLU, SWIGLU_F16) else self.N

    def ldo(self, epi):
        return self.ncols(epi) + self.pad

    def ldr(self):
        return self.N + self.pad

    def route_args(self, epi, cus=CUS, scratch=None, bias=True):
        """the launch as gemm_route's (and library_route's) keyword arguments"""
        return dict(M=self.M, N=self.N, K=self.K, lda=self.lda, ldo=self.ldo(epi), epi=epi, ksplit=self.ksplit, f16=self.f16, tn=self.tn,
                    bias=bias and epi not in (SWIGLU, SWIGLU_SPLIT, SWIGLU_F16), scratch=self.scratch if scratch is None else scratch,
                    few_rows=self.few_rows, norm=self.norm, cus=cus, ldw=self.ldw, ldr=self.ldr())

    def route(self, epi, cus=CUS, scratch=None, bias=True):
        return gemm_route(**self.route_args(epi, cus, scratch, bias))

    def launch_args(self, epi, cus=CUS, scratch=None, bias=True):
        """route_args with the residual and the scale present where the GPU file's launch hands them in (_epilogue_inputs, selection_problem)"""
        return dict(self.route_args(epi, cus, scratch, bias), res=epi in (LS_RES, RES_F32, MUL_AUX) and not self.tn, scale=epi == LS_RES)

    def __repr__(self):
        return self.name


def _ws(ranges, M, N, tile=256):
    return ranges * M * ((N + tile - 1) // tile * tile) * 4


_ASYM, _G256, _T128 = "gemm256_kernel<8,4,ASYM>", "gemm256_kernel<8,4>", "gemm256_kernel<4,2>"
_CM, _RM = "column-major", "row-major"
_TAIL = lambda red: (key(_ASYM, _CM), key(_ASYM, _CM, True, red))                 # noqa: E731
CASES = [
    # the register-staged kernel
    Case("g64", 77, 136, 72, [BIAS, LS_RES, F32, RES_F32, F16, MUL_AUX], key("gemm_kernel<64>"), gauss=[BIAS, GELU, F32]),
    Case("g64-swiglu", 77, 144, 72, [], key("gemm_kernel<64>"), gauss=[SWIGLU, SWIGLU_SPLIT, SWIGLU_F16]),
    Case("g64-f16", 77, 136, 72, [BIAS, F32, RES_F32, F16, MUL_AUX], key("gemm_kernel<64,F16>"), gauss=[F32, F16], f16=True),
    Case("g64-f16-swiglu", 77, 144, 72, [], key("gemm_kernel<64,F16>"), gauss=[SWIGLU_F16, SWIGLU_SPLIT], f16=True),
    Case("g64-stride", 384, 96, 96, [BIAS], key("gemm_kernel<64>"), gauss=[GELU]),                                    # lda = 104: the pointwise kernel refuses the stride
    Case("g64-lo8", 77, 136, 128, [F32, RES_F32, BIAS], key("gemm_kernel<64,LO8>"), gauss=[F32, GELU], ksplit=2),
    Case("g64-ksplit", 77, 136, 360, [F32, BIAS], key("gemm_kernel<64>"), gauss=[F32], ksplit=1),                     # 5.625 K-tiles per half
    Case("g128", 4104, 2048, 72, [BIAS, LS_RES, F32, RES_F32, F16, MUL_AUX], key("gemm_kernel<128>"), gauss=[GELU, SWIGLU, SWIGLU_SPLIT, SWIGLU_F16]),                                 # 33 x 16 = 528 blocks
    Case("g128-f16", 4104, 2048, 72, [BIAS, F32, RES_F32, F16, MUL_AUX], key("gemm_kernel<128,F16>"), gauss=[SWIGLU_SPLIT, SWIGLU_F16], f16=True),
    Case("g128-lo8", 32776, 136, 128, [F32, RES_F32, BIAS], key("gemm_kernel<128,LO8>"), gauss=[GELU], ksplit=2),                                  # 257 x 2 = 514 blocks; a column tile 0.53 full keeps the 256-tile kernel away
    # the pointwise kernel
    Case("pw96", 384, 96, 96, [BIAS], key("pwconv_kernel<96>"), gauss=[GELU], tight=True),
    Case("pw96-second-trip", 128 * 773, 96, 96, [BIAS], key("pwconv_kernel<96>"), gauss=[GELU], tight=True),          # 773 tiles on 768 blocks
    Case("pw192-second-trip", 128 * 259, 192, 192, [BIAS], key("pwconv_kernel<192>"), gauss=[GELU], tight=True),      # 259 tiles on 256 blocks
    # the 256-tile kernel, one pass
    Case("asym-colmajor", 2048, 4096, 128, [BIAS, LS_RES, F32, RES_F32, F16, MUL_AUX], key(_ASYM, _CM), gauss=[GELU, SWIGLU_SPLIT, SWIGLU_F16]),
    Case("asym-colmajor-ksplit", 2048, 4096, 128, [F32, RES_F32, BIAS, LS_RES], key(_ASYM, _CM), gauss=[GELU, SWIGLU_SPLIT, SWIGLU_F16], ksplit=1),
    Case("asym-colmajor-f16", 2048, 4096, 128, [BIAS, F32, RES_F32, F16, MUL_AUX], key("gemm256_kernel<8,4,ASYM,F16>", _CM), gauss=[SWIGLU_F16, SWIGLU_SPLIT], f16=True),
    Case("rowmajor-second-round", 8448, 2560, 128, [BIAS, F32], key(_G256, _RM), gauss=[SWIGLU_F16]),                                     # 33 x 10 = 330 tiles, M > 8192
    Case("group4", 3072, 6912, 128, [BIAS], key(_ASYM, "group_m 4")),                                                 # 12 x 27
    Case("group2", 2560, 8192, 128, [BIAS], key(_ASYM, "group_m 2")),                                                 # 10 x 32
    Case("ragged", 2040, 4104, 128, [BIAS, LS_RES, F32, RES_F32, F16, MUL_AUX], key(_G256, _CM), gauss=[GELU]),                     # 8 x 17 tiles, 8 columns in the last
    Case("ragged-f16", 2040, 4104, 128, [BIAS, F32, RES_F32, F16, MUL_AUX], key("gemm256_kernel<8,4,F16>", _CM), f16=True),
    Case("ragged-rows-swiglu", 2040, 4096, 128, [], key(_G256, _CM), gauss=[SWIGLU_SPLIT]),                           # SwiGLU admits ragged rows only
    Case("ragged-rows-swiglu-f16", 2040, 4096, 128, [], key("gemm256_kernel<8,4,F16>", _CM), gauss=[SWIGLU_SPLIT], f16=True),
    Case("rowmajor-f16", 8448, 2560, 128, [], key("gemm256_kernel<8,4,F16>", _RM), gauss=[SWIGLU_F16], f16=True),     # SWIGLU_F16 wants whole tiles, 320 of them
    Case("ragged-group4", 3064, 6920, 128, [F32, BIAS], key(_G256, "group_m 4")),                                     # 12 x 28 tiles, both edges ragged
    Case("g256-lo8", 2048, 4096, 128, [F32, RES_F32, BIAS], key("gemm256_kernel<8,4,LO8>", _CM), gauss=[GELU], ksplit=2),
    # the 128-tile instance
    Case("t128", 1152, 1920, 512, [BIAS, LS_RES, F32, RES_F32, F16, MUL_AUX], key(_T128, _RM), gauss=[GELU, SWIGLU_SPLIT, SWIGLU_F16]),                                        # 9 x 15 = 135 tiles
    Case("t128-ksplit", 1152, 1920, 512, [RES_F32], key(_T128, _RM), ksplit=1),
    Case("t128-lo8", 1152, 1920, 512, [F32, RES_F32, BIAS], key("gemm256_kernel<4,2,LO8>", _RM), gauss=[GELU], ksplit=2),
    # K ranges on 64-row tiles
    Case("skinny-f32", 77, 136, 1024, [F32, RES_F32], key("gemm_kernel<64>", None, True, "splitk_reduce_kernel"), gauss=[F32], scratch=_ws(8, 77, 136)),
    Case("skinny-ksplit", 77, 136, 360, [RES_F32], key("gemm_kernel<64>", None, True, "splitk_reduce_kernel"), ksplit=1, scratch=_ws(8, 77, 136)),   # the seam inside a range
    Case("skinny-swiglu", 77, 256, 512, [], key("gemm_kernel<64>", None, True, "splitk_reduce_swiglu_kernel"), gauss=[SWIGLU_SPLIT], ksplit=1, scratch=_ws(8, 77, 256)),
    Case("skinny-bf16", 77, 136, 1536, [BIAS, LS_RES], key("gemm_kernel<64>", None, True, "splitk_reduce_bf16_kernel"), gauss=[GELU], scratch=_ws(8, 77, 136)),
    # K ranges on 256-tiles
    Case("splitk", 512, 1024, 2048, [F32, RES_F32], key(_ASYM, _CM, True, "splitk_reduce_kernel"), gauss=[F32], scratch=_ws(8, 512, 1024)),
    Case("splitk-swiglu", 512, 1024, 2048, [], key(_ASYM, _CM, True, "splitk_reduce_swiglu_kernel"), gauss=[SWIGLU_SPLIT], ksplit=1, scratch=_ws(8, 512, 1024)),
    Case("splitk-f16", 512, 1024, 2048, [F32], key("gemm256_kernel<8,4,ASYM,F16>", _CM, True, "splitk_reduce_kernel"), f16=True, scratch=_ws(8, 512, 1024)),
    Case("splitk-lo8", 512, 1024, 2048, [F32], key("gemm256_kernel<8,4,LO8>", _CM, True, "splitk_reduce_kernel"), ksplit=2, scratch=_ws(8, 512, 1024)),
    Case("splitk-ragged", 1160, 904, 2048, [F32, RES_F32], key(_G256, _CM, True, "splitk_reduce_kernel"), scratch=_ws(8, 1160, 904)),   # M > 1024: not the few-row form
    Case("splitk-ragged-f16", 1160, 904, 2048, [F32], key("gemm256_kernel<8,4,F16>", _CM, True, "splitk_reduce_kernel"), f16=True, scratch=_ws(8, 1160, 904)),
    Case("splitk-short-scratch", 512, 1024, 8192, [F32], key(_ASYM, _CM, True, "splitk_reduce_kernel"), scratch=_ws(3, 512, 1024)),     # room for 3 ranges where the model wants 8
    Case("tail", 1024, 17408, 1024, [RES_F32], _TAIL("splitk_reduce_kernel"), ksplit=1, scratch=_ws(4, 1024, 1024)),                    # 272 tiles, cut at column 16384
    Case("tail-swiglu", 1024, 17408, 1024, [], _TAIL("splitk_reduce_swiglu_kernel"), gauss=[SWIGLU_SPLIT], ksplit=1, scratch=_ws(4, 1024, 1024)),
    # TN
    Case("tn", 520, 264, 192, [F32], key("gemm256_kernel<8,4,TN>", _CM), gauss=[F32], tn=True),
    Case("tn-f16", 520, 264, 192, [F32], key("gemm256_kernel<8,4,F16,TN>", _CM), tn=True, f16=True),
    Case("tn-ranges", 520, 264, 2048, [F32], key("gemm256_kernel<8,4,TN>", _CM, True, "splitk_reduce_kernel"), gauss=[F32], tn=True, scratch=_ws(8, 520, 264)),
    Case("tn-ranges-f16", 520, 264, 2048, [F32], key("gemm256_kernel<8,4,F16,TN>", _CM, True, "splitk_reduce_kernel"), tn=True, f16=True, scratch=_ws(8, 520, 264)),
    # the RMSNorm that follows (fv_op_gemm_norm)
    Case("norm-row-256", 4096, 896, 2432, [RES_F32], key(_ASYM, _RM, True, "splitk_reduce_norm_row_kernel", "fused"), gauss=[RES_F32], ksplit=1, norm=True,
         scratch=_ws(8, 4096, 896)),
    Case("norm-wave-256", 4096, 896, 2432, [RES_F32], key(_ASYM, _RM, True, "splitk_reduce_norm_kernel", "fused"), gauss=[RES_F32], ksplit=1, norm=True, few_rows=0,
         scratch=_ws(8, 4096, 896)),
    Case("norm-separate-256", 4096, 896, 2432, [RES_F32], key("gemm_kernel<64>", None, False, None, "separate"), ksplit=1, norm=True),
    Case("norm-row-skinny", 77, 896, 1024, [RES_F32, F32], key("gemm_kernel<64>", None, True, "splitk_reduce_norm_row_kernel", "fused"), gauss=[RES_F32], ksplit=1,
         norm=True, scratch=_ws(8, 77, 896)),
    Case("norm-wave-ragged", 77, 896, 1024, [RES_F32], key(_G256, _CM, True, "splitk_reduce_norm_kernel", "fused"), gauss=[RES_F32], ksplit=1, norm=True, few_rows=0,
         scratch=_ws(8, 77, 896)),
    Case("norm-separate-skinny", 77, 896, 1024, [RES_F32], key("gemm_kernel<64>", None, False, None, "separate"), gauss=[RES_F32], ksplit=1, norm=True),
]
CASE = {c.name: c for c in CASES}


def covered_epilogues(cus=CUS):
    """kernel -> the epilogues the case list runs through it in ONE pass (behind K ranges the GEMM kernel stores raw sums and the reducer owns the epilogue)"""
    out = {}
    for c in CASES:
        for epi in set(c.epis) | set(c.gauss):
            r = c.route(epi, cus)
            for x in (r if isinstance(r, list) else [r]):
                if not refused(x) and x["splits"] == 1:
                    out.setdefault(x["kernel"], set()).add(epi)
    return out


def covered_reducer_epilogues(cus=CUS):
    out = {}
    for c in CASES:
        for epi in set(c.epis) | set(c.gauss):
            r = c.route(epi, cus)
            for x in (r if isinstance(r, list) else [r]):
                if not refused(x) and x["reducer"]:
                    out.setdefault(x["reducer"], set()).add(epi)
    return out


# What every instance's own epilogue code admits AND an op-level entry point can express: the CPU file asserts that the case list runs exactly these.
_BF16_OPS = {BIAS, GELU, LS_RES, RES_F32, F32, SWIGLU_SPLIT, SWIGLU_F16, F16, MUL_AUX}
_F16_OPS = {BIAS, RES_F32, F32, SWIGLU_SPLIT, SWIGLU_F16, F16, MUL_AUX}                    # check_gemm refuses GELU, LS_RES, SWIGLU with fp16 operands
_LO8_OPS = {BIAS, GELU, RES_F32, F32}
EPILOGUES = {
    "gemm_kernel<64>": _BF16_OPS | {SWIGLU}, "gemm_kernel<128>": _BF16_OPS | {SWIGLU},     # plain SWIGLU: the register-staged kernel only (gemm_glds_tile returns 0)
    "gemm_kernel<64,F16>": _F16_OPS, "gemm_kernel<128,F16>": _F16_OPS,
    "gemm_kernel<64,LO8>": _LO8_OPS, "gemm_kernel<128,LO8>": _LO8_OPS,
    "gemm256_kernel<8,4>": _BF16_OPS, "gemm256_kernel<8,4,ASYM>": _BF16_OPS, "gemm256_kernel<4,2>": _BF16_OPS,
    "gemm256_kernel<8,4,F16>": _F16_OPS, "gemm256_kernel<8,4,ASYM,F16>": _F16_OPS,
    "gemm256_kernel<8,4,LO8>": _LO8_OPS, "gemm256_kernel<4,2,LO8>": _LO8_OPS,
    "gemm256_kernel<8,4,TN>": {F32}, "gemm256_kernel<8,4,F16,TN>": {F32},
    "pwconv_kernel<96>": {BIAS, GELU}, "pwconv_kernel<192>": {BIAS, GELU},
}
REDUCER_EPILOGUES = {"splitk_reduce_kernel": {F32, RES_F32}, "splitk_reduce_norm_kernel": {RES_F32}, "splitk_reduce_norm_row_kernel": {F32, RES_F32},
                     "splitk_reduce_bf16_kernel": {BIAS, GELU, LS_RES}, "splitk_reduce_swiglu_kernel": {SWIGLU_SPLIT}}
# Admitted by launch_gemm but deliberately in no case of this suite, and why
OMITTED = {
    "MUL_GELUP (every instance that admits the fp16-output epilogues)":
        "reachable through fv_op_gemm_f16 / fv_op_gemm_f16_gelup; csrc/common.h documents no error for mul_gelu_grad8's gelu' from which a per-element bound could "
        "be derived, and it is no linear epilogue; tests/test_gpu_ops.py test_fused_convffn32_stash_and_gelup_epilogue holds it against the oracle",
    "GELU_GRAD": "needs GemmArgs::stash, which no fv_op_* entry point that takes an epilogue number hands in (the launch is refused)",
    "hi + lo8 operands with SWIGLU / SWIGLU_SPLIT / SWIGLU_F16":
        "SWIGLU_SPLIT's lo half leaves as fp8 bytes, a fourth output format; tests/test_gpu_ops.py test_gemm_hi_lo8_operands decodes it on the register-staged and "
        "the 256-tile kernel.  The other two are admitted by the dispatcher and used by no caller",
    "hi + lo8 operands with LS_RES": "fv_op_gemm_lo8 takes no scale: no entry point",
    "TN with RES_F32": "fv_op_gemm_tn passes FV_EPI_F32 and no residual: no entry point (which is also why the refusal 'TN with a non-fp32 epilogue' cannot be sent)",
    "splitk_reduce_norm_kernel with F32 (no residual)": "the same code as RES_F32 with res == nullptr, which splitk_reduce_norm_row_kernel's F32 case runs",
}


def covered(cus=CUS):
    """(kernels, reducers, walks, norm placements) the case list reaches on a device of `cus` CUs"""
    ks, rs, ws, ns = set(), set(), set(), set()
    for c in CASES:
        for epi in set(c.epis) | set(c.gauss):
            r = c.route(epi, cus)
            for x in (r if isinstance(r, list) else [r]):
                if refused(x):
                    continue
                ks.add(x["kernel"]); rs.add(x["reducer"]); ws.add(x["walk"]); ns.add(x["norm"])
    return ks, rs - {None}, ws - {None}, ns - {None}


# launches that must be refused: (what, keyword arguments of gemm_route); the GPU file sends the same launch and expects a non-zero code and an untouched output.
# (A misaligned pointer is the one refusal the mirror cannot see: the GPU file adds it by hand.  "TN with a non-fp32 epilogue" is refused by check_gemm, but
# fv_op_gemm_tn always passes FV_EPI_F32: no entry point can send it.)
REFUSED = [
    ("K % 8", dict(M=64, N=64, K=68, lda=72, epi=BIAS)),
    ("lda % 8", dict(M=64, N=64, K=64, lda=68, epi=BIAS)),
    ("N % 8", dict(M=64, N=68, K=64, lda=64, ldo=72, epi=BIAS)),
    ("lda < K", dict(M=64, N=64, K=64, lda=56, epi=BIAS)),
    ("ldo < N", dict(M=64, N=64, K=64, lda=64, ldo=56, epi=BIAS)),
    ("ldo % 8 (bf16 output)", dict(M=64, N=64, K=64, lda=64, ldo=68, epi=BIAS)),
    ("epilogue 6", dict(M=64, N=64, K=64, lda=64, epi=6)),
    ("f16 with GELU", dict(M=64, N=64, K=64, lda=64, epi=GELU, f16=True)),
    ("f16 with LS_RES", dict(M=64, N=64, K=64, lda=64, epi=LS_RES, f16=True)),
    ("f16 with SWIGLU", dict(M=64, N=64, K=64, lda=64, epi=SWIGLU, f16=True)),
    ("ksplit with an fp16-output epilogue", dict(M=64, N=64, K=64, lda=128, epi=F16, ksplit=1)),
    ("lo8 with K % 128", dict(M=64, N=64, K=64, lda=128, epi=F32, ksplit=2)),
    ("TN with K % 64", dict(M=64, N=64, K=96, lda=64, ldw=64, epi=F32, tn=True)),
    ("norm with ldo != N", dict(M=64, N=64, K=64, lda=128, ldo=72, epi=F32, ksplit=1, norm=True)),
    ("norm with a bf16 epilogue", dict(M=64, N=64, K=64, lda=128, epi=BIAS, ksplit=1, norm=True)),
]


# ------------------------------------------------------------------------------------------------ inputs
SENT = 1.0e4            # what pad columns and the rows past M / N hold: finite (the clamped staging re-reads the last valid row, nothing may read past it)
GUARD_ROWS = 8
EXACT_BITS = 22         # every partial sum stays below 2^22 q: two bits under fp32's 24 (the matrix core's internal alignment is not documented)


def _store_dtype(c):
    return torch.float16 if c.f16 else torch.bfloat16


def exact_ranges(c, epi):
    """(max |A|, max |W|, bias range, max |res|, q, limit): integer operands whose every partial sum is a multiple of q below limit = 2^22 q (2^21 q under LS_RES,
    whose scales of 1/2, 1, 2 cost one bit at either end).  Split operands: hi integers, lo = j 2^-8, so q = 2^-8."""
    q = 2.0 ** -8 if c.ksplit else 1.0
    limit = 2.0 ** (EXACT_BITS - (1 if epi == LS_RES else 0)) * q
    if epi in (F16, MUL_AUX):
        b_lo, b_hi = 2100, 8000                       # fp16 keeps integers up to 2048: beyond, most sums need rounding
    elif epi in F32_EPIS:
        b_lo, b_hi = 0, 4000
    else:
        b_lo, b_hi = 300, 2000                        # bf16 keeps integers up to 256
    rmax = 4000 if epi == RES_F32 else (255 if epi == LS_RES else (4 if epi == MUL_AUX else 0))
    extras = b_hi + (rmax if epi in (RES_F32, LS_RES) else 0)
    if epi == LS_RES:
        extras = 2 * b_hi + rmax
    if epi == MUL_AUX:
        limit = min(limit, 60000.0 / 4)               # |acc + bias| * |aux| stays inside fp16's range
    prod = int((limit - extras) // ((2 if epi == LS_RES else 1) * c.ktotal))
    lim = 7 if c.ksplit == 2 else 8                   # e4m3 keeps the integers up to 7 times a power of two: W8 = W exactly
    w = max(1, min(lim, int(math.isqrt(prod))))
    a = max(1, min(8, prod // w))
    return a, w, (b_lo, b_hi), rmax, q, limit


def exact_budget(c, epi):
    """the issue's figure: (max|A| max|W| K_total + |bias| + |res|) / q, which has to stay below 2^22 (2^21 under LS_RES)"""
    a, w, (_, b_hi), rmax, q, limit = exact_ranges(c, epi)
    amax = max(a, 1) if c.ksplit else a               # a lo element is below 1 in magnitude
    total = amax * w * c.ktotal + (2 * b_hi + rmax if epi == LS_RES else b_hi + (rmax if epi == RES_F32 else 0))
    return total / q, limit / q


def _rint(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _signed(shape, lo, hi, g):
    return _rint(shape, lo, hi, g) * (2 * torch.randint(0, 2, shape, generator=g).double() - 1)


class Problem:
    """Host side of one launch.  Stored tensors carry their pads: A [rows + 8][lda] (TN: [K][lda]), W [N + 8][K] (TN: [K][ldw]); rows past M / N and pad columns
    hold +-SENT.  Aval [M][K] / Alo [M][K] (the lo8 remainder, else folded into Aval) / Wval [N][K] / W8val are the float64 VALUES of what is stored."""

    def __init__(self, c, epi):
        self.c, self.epi = c, epi
        self.bias = self.scale = self.res = self.Alo = self.W8val = self.normw = None


def _sentinels(shape, g):
    return SENT * (2 * torch.randint(0, 2, shape, generator=g).double() - 1)


def e4m3(t):
    return t.to(torch.float32).to(torch.float8_e4m3fn)


def _pack(p, hi, lo, W, g):
    """values -> the stored operands.  hi, lo [M][K] (lo None: one operand), W [N][K]; TN: hi is [K][M], W [K][N]"""
    c, dt = p.c, _store_dtype(p.c)
    if c.tn:
        A = _sentinels((c.K, c.lda), g); A[:, :c.M] = hi
        Ws = _sentinels((c.K, c.ldw), g); Ws[:, :c.N] = W
        p.A, p.W = A.to(dt), Ws.to(dt)
        p.Aval, p.Wval = p.A[:, :c.M].double().t().contiguous(), p.W[:, :c.N].double().t().contiguous()
        return p
    A = _sentinels((c.M + GUARD_ROWS, c.lda), g)
    A[:c.M, :c.K] = hi
    if c.ksplit == 1:
        A[:c.M, c.K:2 * c.K] = lo
    p.A = A.to(dt)
    if c.ksplit == 2:                                   # K fp8 bytes of lo x 2^8 from byte 2K of the row; the rest of the 2K-wide row: sentinel bytes (0x7e = 448)
        raw = p.A.view(torch.uint8)                     # [rows][2 lda]
        raw[:c.M, 2 * c.K:4 * c.K] = 0x7e
        raw[:c.M, 2 * c.K:3 * c.K] = e4m3(lo * 256.0).view(torch.uint8)
        p.Alo = raw[:c.M, 2 * c.K:3 * c.K].contiguous().view(torch.float8_e4m3fn).double() / 256.0
        p.W8val = e4m3(W * 64.0).double() / 64.0        # the GPU file replaces this by what fv_op_lo8_pack stored
    Ws = _sentinels((c.N + GUARD_ROWS, c.K), g); Ws[:c.N] = W
    p.W = Ws.to(dt)
    st = p.A[:c.M].double()
    p.Aval = st[:, :c.K] + (st[:, c.K:2 * c.K] if c.ksplit == 1 else 0.0)
    p.Wval = p.W[:c.N].double()
    return p


def _epilogue_inputs(p, g, bias, rmax, integer):
    """bias / scale / residual / aux as the epilogue needs them; integer: the exact class's values"""
    c, epi = p.c, p.epi
    if epi not in (SWIGLU, SWIGLU_SPLIT, SWIGLU_F16):
        p.bias = (_signed((c.N,), bias[0], bias[1], g) if integer else torch.randn(c.N, generator=g).double() * 0.1).float()
    if epi == LS_RES:
        p.scale = (2.0 ** _rint((c.N,), -1, 1, g) if integer else torch.rand(c.N, generator=g).double() * 0.3 + 0.05).float()
    if epi in (LS_RES, RES_F32, MUL_AUX) and not c.tn:
        r = _sentinels((c.M, c.ldr()), g)
        r[:, :c.N] = (_signed((c.M, c.N), 1 if epi == MUL_AUX else 0, rmax, g) if integer else torch.randn(c.M, c.N, generator=g).double())
        p.res = r.to(torch.float32 if epi == RES_F32 else (torch.float16 if epi == MUL_AUX else torch.bfloat16))
    if c.norm:
        p.normw = (1.0 + 0.3 * torch.randn(c.N, generator=g)).float()
    return p


def exact_problem(c, epi, *seed):
    g = gen(c.M, c.N, c.K, epi, 11, *seed)
    a, w, bias, rmax, q, _ = exact_ranges(c, epi)
    shape = (c.K, c.M) if c.tn else (c.M, c.K)
    hi = _rint(shape, -a, a, g)
    lo = _rint(shape, -7, 7, g) / 256.0 if c.ksplit == 2 else (_rint(shape, -255, 255, g) / 256.0 if c.ksplit else None)
    W = _rint((c.K, c.N) if c.tn else (c.N, c.K), -w, w, g)
    return _epilogue_inputs(_pack(Problem(c, epi), hi, lo, W, g), g, bias, rmax, True)


def gauss_problem(c, epi, *seed):
    g = gen(c.M, c.N, c.K, epi, 12, *seed)
    dt = _store_dtype(c)
    shape = (c.K, c.M) if c.tn else (c.M, c.K)
    x = torch.randn(shape, generator=g) * 0.7
    hi = x.to(dt).double()
    lo = (x.double() - hi) if c.ksplit else None        # _pack rounds it to the lo half's format
    W = torch.randn((c.K, c.N) if c.tn else (c.N, c.K), generator=g).double() / math.sqrt(c.K)
    return _epilogue_inputs(_pack(Problem(c, epi), hi, lo, W, g), g, None, 0, False)


def selection_weights(N, K, lo8=False):
    """W[n][k] = ((131 n + 71 k) mod 509) - 254: bf16 and fp16 values, distinct along k inside any 64-tile (71 k mod 509 has no repeat within 509 steps).
    lo8: the weights' fp8 copy is e4m3(64 W), which would saturate nearly all of those at +-7.  There W[n][k] = +-2^e (1 + m / 8) / 64 with (sign, e, m) from
    j = (131 n + 71 k) mod 238 -- e4m3's 119 normal magnitudes 2^-6 .. 448 and both signs, so that W8 = W exactly and still bf16 values -- distinct along k inside
    any 128-deep fp8 step (71 k mod 238 has no repeat within 238 steps)"""
    n, k = torch.arange(N).view(N, 1), torch.arange(K).view(1, K)
    if not lo8:
        return ((131 * n + 71 * k) % 509 - 254).double()
    j = (131 * n + 71 * k) % 238
    mag, sign = j % 119, 1.0 - 2.0 * (j // 119).double()
    return sign * torch.ldexp(1.0 + (mag % 8).double() / 8.0, mag // 8 - 6) / 64.0


def selection_launches(c):
    """how many launches it takes for pi to cover every k of both halves: rows with m % 11 == 7 select nothing (their output is +0), the others take the
    positions in turn"""
    nsel = sum(1 for m in range(c.M) if m % 11 != 7)
    return (c.ktotal + nsel - 1) // nsel


def selection_problem(c, epi, launch):
    """(problem, pi): row m of A is one-hot at position pi[m] of [hi | lo] (-1: an empty row).  No bias (a residual of zeros where the epilogue wants one)."""
    g = gen(c.M, c.N, c.K, 13)
    rows = [m for m in range(c.M) if m % 11 != 7]
    pi = torch.full((c.M,), -1, dtype=torch.int64)
    pi[rows] = (torch.arange(len(rows)) + launch * len(rows)) % c.ktotal
    hi, lo = torch.zeros(c.M, c.K, dtype=torch.float64), (torch.zeros(c.M, c.K, dtype=torch.float64) if c.ksplit else None)
    sel = pi >= 0
    first = sel & (pi < c.K)
    hi[first.nonzero().flatten(), pi[first]] = 1.0
    if c.ksplit:
        second = sel & (pi >= c.K)
        lo[second.nonzero().flatten(), pi[second] - c.K] = 1.0        # lo8: the byte of 256, read as 256 / 2^8
    W = selection_weights(c.N, c.K, c.ksplit == 2)
    p = _pack(Problem(c, epi), hi.t().contiguous() if c.tn else hi, lo, W.t().contiguous() if c.tn else W, g)
    if epi == RES_F32:
        p.res = torch.zeros(c.M, c.ldr(), dtype=torch.float32)
    return p, pi


def selection_expected(p, pi):
    """W[n][pi(m)] -- from the lo8 half: the weights' fp8 copy -- and +0 on the empty rows"""
    c = p.c
    k = pi.clamp_min(0) % c.K
    want = p.Wval[:, k].t().clone()
    if c.ksplit == 2:
        second = pi >= c.K
        want[second] = p.W8val[:, k[second]].t()
    want[pi < 0] = 0.0
    return want


# ------------------------------------------------------------------------------------------------ references (float64) and checks
def reference(p, cols=None):
    """(pre, A_abs) [M][len(cols)]: the float64 product on the stored values, and sum |a w|; cols: a column subset"""
    W = p.Wval if cols is None else p.Wval[cols]
    pre, ab = p.Aval @ W.t(), p.Aval.abs() @ W.abs().t()
    if p.Alo is not None:
        W8 = p.W8val if cols is None else p.W8val[cols]
        pre, ab = pre + p.Alo @ W8.t(), ab + p.Alo.abs() @ W8.abs().t()
    return pre, ab


def swiglu_halves(t):
    """[M][N] accumulator columns -> gate, up [M][N / 2]: W's rows come as 8 gate | 8 up"""
    M, N = t.shape
    v = t.view(M, N // 16, 2, 8)
    return v[:, :, 0].reshape(M, N // 2), v[:, :, 1].reshape(M, N // 2)


def exact_expected(p):
    """the exact class's output VALUES in float64 (every one an fp32 value): the caller rounds to the output format"""
    pre, _ = reference(p)
    c, epi = p.c, p.epi
    v = pre + (p.bias.double() if p.bias is not None else 0.0)
    if epi == RES_F32:
        v = v + p.res[:, :c.N].double()
    elif epi == LS_RES:
        v = p.res[:, :c.N].double() + p.scale.double() * v
    elif epi == MUL_AUX:
        v = v * p.res[:, :c.N].double()
    return v


def out_dtype(epi):
    return torch.float32 if epi in F32_EPIS else (torch.float16 if epi in F16_OUT_EPIS or epi == SWIGLU_F16 else torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_bits(got, want64, what):
    """got in its output format; want64 float64 values that fp32 holds exactly: equal to their round-to-nearest-even, bit for bit (an unwritten NaN, a -0 fail)"""
    w32 = want64.to(torch.float32)
    assert bool((w32.double() == want64).all()), f"{what}: the expected values are not fp32 values (the class's budget is broken)"
    want = w32.to(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}")


def rounding_census(want64, dtype):
    """(fraction of outputs that need rounding, fraction that are ties) in the output format"""
    r = want64.to(torch.float32).to(dtype).double()
    need = r != want64
    tie = need & ((want64 - r).abs() == half_ulp(want64, dtype))
    return float(need.double().mean()), float(tie.double().mean())


def half_ulp(v, dtype):
    """half the spacing of the format's values around |v|: bf16 8 significant bits, fp16 11 (subnormal step 2^-24), fp32: 0 (the bound's D covers it)"""
    if dtype == torch.float32:
        return torch.zeros_like(v.double())
    if dtype == torch.bfloat16:
        return bf16_half_ulp(v)
    v = v.double().abs()
    _, e = torch.frexp(v)
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), (e - 12).clamp_min(-25)), torch.zeros_like(v))


def splits_of(route):
    return max(x["splits"] for x in (route if isinstance(route, list) else [route]))


SILU_REL = 2.0 ** -22       # the hardware's exponential and reciprocal (1 ulp each), relative to the result
SILU_ERR = 6.0e-7           # |float32 emulation of silu_f - float64 silu| / |silu| over |x| <= 8: measured 5.5e-7 on the CPU (test_silu_emulation_error); it grows
SILU_RANGE = 8.0            # with |x| (the product x log2 e is rounded before the exponential), so the Gaussian class asserts that its gates stay inside


def silu64(x):
    return x * torch.sigmoid(x)


def silu_emulated(x):
    """float32 emulation of silu_f (csrc/common.h): x * rcp(1 + __expf(-x)), __expf(t) = exp2(t log2 e) with the product rounded to float32; correctly rounded
    exp2 and division stand in for the hardware's approximations (SILU_REL covers those)"""
    x = x.to(torch.float32)
    return x * (1.0 / (1.0 + torch.exp2(-x * torch.tensor(1.4426950408889634, dtype=torch.float32))))


def gauss_check(p, got, splits, cols=None, what=""):
    """per element, against float64 on the stored values.  got: the output [M][ncols (of cols)] in its format (SWIGLU_SPLIT: the (hi, lo) pair).  Returns the worst
    fraction of the bound.  cols (a subset of ACCUMULATOR columns, whole groups of 16 under SwiGLU) restricts reference and output alike."""
    c, epi = p.c, p.epi
    pre, ab = reference(p, cols)
    sub = (lambda t: t) if cols is None else (lambda t: t[cols])
    if p.bias is not None:
        pre = pre + sub(p.bias.double())
    A = ab + (sub(p.bias.double()).abs() if p.bias is not None else 0.0)
    res = None if p.res is None else (p.res[:, :c.N].double() if cols is None else p.res[:, :c.N].double()[:, cols])
    if epi == RES_F32:
        pre, A = pre + res, A + res.abs()
    D = (c.ktotal + splits + 4) * 2.0 ** -23 * A
    dt = out_dtype(epi)
    if epi in (F32, RES_F32, BIAS, F16):
        ref = pre
    elif epi == GELU:
        ref, D = gelu_erf(pre), GELU_ERR["gelu2_n"] + GELU_SLOPE * D
    elif epi == LS_RES:
        s = sub(p.scale.double())
        ref, D = res + s * pre, s * D + 2.0 ** -23 * (res.abs() + (s * pre).abs() + s * D)        # the multiply and the add round once each
    elif epi in (SWIGLU, SWIGLU_SPLIT, SWIGLU_F16):
        (gt, up), (Dg, Du) = swiglu_halves(pre), swiglu_halves(D)
        sg = silu64(gt)
        assert float(gt.abs().max()) <= SILU_RANGE
        # |silu'| <= 1.1; silu_f's own error (SILU_ERR + SILU_REL, relative to |silu|); the product's rounding
        Ds = 1.1 * Dg + (SILU_ERR + SILU_REL) * sg.abs()
        ref = sg * up
        D = Ds * (up.abs() + Du) + sg.abs() * Du + 2.0 ** -23 * (ref.abs() + Ds * up.abs())
        if epi == SWIGLU_F16:
            ref, D = ref / 16.0, D / 16.0
    else:
        raise AssertionError(f"no Gaussian bound for epilogue {epi}")
    if epi == SWIGLU_SPLIT:
        hi, lo = got[0].double(), got[1].double()
        assert bool(torch.isfinite(hi).all() and torch.isfinite(lo).all()), f"{what}: non-finite output"
        bound = D + 2.0 ** -17 * ref.abs()
        frac = ((hi + lo - ref).abs() / bound).max()
        near = lo.abs() <= bf16_half_ulp(hi)
        assert bool(near.all()), f"{what}: |lo| exceeds half an ulp of hi at {tuple(int(v) for v in (~near).nonzero()[0])}: hi is not the nearest bf16"
    else:
        g = got.double()
        assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
        bound = half_ulp(ref.abs() + D, dt) + D
        frac = ((g - ref).abs() / bound).max()
    frac = float(frac)
    print(f"[gemm gauss] {what}: worst |got - ref| / bound = {frac:.3f}")
    assert frac <= 1.0, f"{what}: {frac:.3f} of the derived bound"
    return frac


# RMSNorm behind the GEMM: y (+ y_lo) against float64 RMSNorm of the RETURNED out.  The kernel's operations on a row of N values: N squares and a sum of them
# (a lane's chain of N / 64 additions, six levels of the wave's tree, up to two more across waves: relative error (N / 64 + 9) 2^-24 on a sum of positive
# terms, the squares' own rounding included), the division by N and the eps add (2), the reciprocal square root (halves what is under it; the hardware's own
# error 2^-22), two multiplies (2).  The hi | lo pair then keeps 16 bits: 2^-17 relative.  Together, for N = 896: (25 / 2 + 4 + 2) 2^-24 + 2^-17 = 1.14 2^-17,
# inside the 2^-16 that test_rmsnorm_output_forms allows the stand-alone kernel.
def norm_rel_bound(N):
    return ((N / 64 + 9 + 2) / 2 + 4 + 2) * 2.0 ** -24 + 2.0 ** -17


def norm_check(out, y, ylo, w, eps, what=""):
    x = out.double()
    ref = w.double() * x * torch.rsqrt((x * x).mean(dim=1, keepdim=True) + eps)
    hi, lo = y.double(), ylo.double()
    bound = norm_rel_bound(x.shape[1]) * ref.abs() + 2.0 ** -140
    frac = float(((hi + lo - ref).abs() / bound).max())
    print(f"[gemm norm] {what}: worst |hi + lo - ref| / bound = {frac:.3f} (bound {norm_rel_bound(x.shape[1]):.3e} |ref|)")
    assert norm_rel_bound(x.shape[1]) <= 2.0 ** -16
    assert frac <= 1.0, f"{what}: {frac:.3f} of the counted bound"
    assert bool((lo.abs() <= bf16_half_ulp(hi)).all()), f"{what}: |lo| exceeds half an ulp of hi"
    return frac


def sample_cols(c, epi, route, limit=2.0e9):
    """None (all columns) where the float64 reference is cheap, else ~512 accumulator columns in whole groups of 16: both ends, the middle, both sides of a cut"""
    if float(c.M) * c.N * c.ktotal <= limit:
        return None
    marks = [0, c.N // 2, c.N - 64]
    if isinstance(route, list):
        marks += [route[0]["cols"][1] - 64, route[0]["cols"][1]]
    cols = sorted({n for m in marks for n in range(m // 16 * 16, min(c.N, m // 16 * 16 + 64))})
    return torch.tensor(cols)


def out_cols(epi, cols):
    """accumulator columns (whole 16-groups) -> the output columns they produce"""
    if epi not in (SWIGLU, SWIGLU_SPLIT, SWIGLU_F16):
        return cols
    g = cols.view(-1, 16)[:, :8]
    return (g // 16 * 8 + g % 16).flatten()


# ------------------------------------------------------------------------------------------------ float32 / bf16 emulation, with defects to plant
def emulate(p, *, truncate=False, double_round=False, swap_k=None, drop_lo_tail=False, late_row=None, splits=1):
    """The kernels' arithmetic on the CPU for the NT forms with bf16 operands: float32 products summed K-tile by K-tile (64 deep, the hi half then the lo half),
    `splits` K ranges added in order, the epilogue in float32, one rounding to the output format.  Returns the output [M][ldo] in a NaN-filled buffer
    (SWIGLU_SPLIT: hi | lo side by side).  Defects:
      truncate      the bf16 output is truncated instead of rounded
      double_round  LS_RES rounds scale * (acc + bias) to bf16 before the residual add
      swap_k        (k1, k2): A's k-slots k1 and k2 of one 32-deep step change places (W's do not)
      drop_lo_tail  the lo half's last K-tile is never added
      late_row      row r is written one row late (row r stays unwritten, row r + 1 holds r's values)"""
    c, epi = p.c, p.epi
    assert not c.tn and not c.f16 and c.ksplit != 2
    A = p.A[:c.M].float()
    W = p.W[:c.N].float()
    halves = [A[:, :c.K]] + ([A[:, c.K:2 * c.K]] if c.ksplit else [])
    if swap_k is not None:
        k1, k2 = swap_k
        assert k1 // 32 == k2 // 32
        h = halves[0].clone()
        h[:, [k1, k2]] = h[:, [k2, k1]]
        halves[0] = h
    tiles = []
    nk1 = (c.K + 63) // 64
    for hidx, h in enumerate(halves):
        for t in range(nk1):
            if drop_lo_tail and hidx == 1 and t == nk1 - 1:
                continue
            tiles.append((h[:, 64 * t:64 * t + 64], W[:, 64 * t:64 * t + 64]))
    nk = len(tiles)
    parts = []
    for s in range(splits):
        acc = torch.zeros(c.M, c.N, dtype=torch.float32)
        for a, w in tiles[s * nk // splits:(s + 1) * nk // splits]:
            acc = acc + a @ w.t()
        parts.append(acc)
    v = parts[0]
    for q in parts[1:]:
        v = v + q
    if p.bias is not None:
        v = v + p.bias
    rnd = bf16_truncate if truncate else bf16_round
    ldo = c.ldo(epi)
    out = torch.full((c.M, ldo), float("nan"), dtype=out_dtype(epi))
    if epi in (F32, RES_F32):
        y = v + p.res[:, :c.N] if epi == RES_F32 else v
    elif epi == BIAS:
        y = rnd(v)
    elif epi == GELU:
        y = rnd(gelu2_n_emulated(v))
    elif epi == LS_RES:
        sv = p.scale * v
        y = rnd(p.res[:, :c.N].float() + (bf16_round(sv) if double_round else sv))
    elif epi in (SWIGLU, SWIGLU_SPLIT):
        gt, up = swiglu_halves(v)
        o = silu_emulated(gt) * up
        hi = rnd(o)
        y = torch.cat([hi, bf16_round(o - hi)], dim=1) if epi == SWIGLU_SPLIT else hi
    else:
        raise AssertionError(epi)
    if late_row is not None:
        y = y.clone()
        y[late_row + 1] = y[late_row]
        y[late_row] = float("nan")
    out[:, :y.shape[1]] = y.to(out.dtype)
    return out
