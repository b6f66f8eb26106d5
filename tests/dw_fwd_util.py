"""CPU-only helpers of the depthwise-forward op tests (tests/test_gpu_dw_forward.py, tests/test_dw_forward_reference_host.py): int64 and float64 references, the
stride-2 Toeplitz table, a mirror of the four forward launchers' route selection, the case tables both files read, the input classes, the checks themselves (so the
CPU file can run them against a deliberately broken arithmetic) and a float32 / bf16 emulation of the kernels' arithmetic with defects that can be planted.

Layouts as the kernels take them: activations NHWC bf16, VALU taps tap-major [k*k][Ci*mult] fp32 with out-channel co = ci*mult + q, MFMA taps as bf16 Toeplitz tables.
Everything here works in NCHW with torch's grouped-conv weight (Co, 1, k, k); nhwc() / nchw() / tap_major() convert.

The route mirror restates launch_dwconv, launch_dwconv_mfma, launch_dwconv_s2_mfma and launch_dwconv_pair of csrc/tower_kernels.hip for the PRODUCT build
(DW_TH7 = 8, no DW_MARCH3, DP_DEFAULT_GEO = 1): first match wins, block and segment arithmetic included."""
import math

import torch
import torch.nn.functional as F

from dw_bwd_util import INSTANCES, conv_weight, nchw, nhwc, out_size, toeplitz  # noqa: F401  (re-exported: the forward tests read them from here)


def tap_major(w, k):
    """torch's (Co, 1, k, k) -> the VALU kernels' tap-major [k*k][Co] (the inverse of conv_weight)"""
    return w.reshape(w.shape[0], k * k).t().contiguous()


# ------------------------------------------------------------------------------------------------ Toeplitz table of the stride-2 kernel
def toeplitz_s2(w):
    """[2C,1,7,7] -> the table of fv_op_dwconv_s2_mfma: [C/16][e][ky][m][16 ch][4 i][4 kk] = w[2(16g+ch)+e][ky][4m+kk-2i]."""
    C = w.shape[0] // 2
    wv = w.view(C // 16, 16, 2, 7, 7)                       # [g][ch][e][ky][kx]
    t = torch.zeros(C // 16, 2, 7, 4, 16, 4, 4)
    for m in range(4):
        for i in range(4):
            for kk in range(4):
                kx = 4 * m + kk - 2 * i
                if 0 <= kx < 7:
                    t[:, :, :, m, :, i, kk] = wv[:, :, :, :, kx].permute(0, 2, 3, 1)
    return t


def toeplitz_s2_definition(w):
    """the same table, one element at a time from the definition in include/fastvla_hip_testops.h (slow: for the CPU test's small C only)"""
    C = w.shape[0] // 2
    t = torch.zeros(C // 16, 2, 7, 4, 16, 4, 4)
    for g in range(C // 16):
        for e in range(2):
            for ky in range(7):
                for m in range(4):
                    for ch in range(16):
                        for i in range(4):
                            for kk in range(4):
                                kx = 4 * m + kk - 2 * i
                                if 0 <= kx < 7:
                                    t[g, e, ky, m, ch, i, kk] = w[2 * (16 * g + ch) + e, 0, ky, kx]
    return t


# ------------------------------------------------------------------------------------------------ references
def conv_int(x, w, b, k, stride, mult):
    """x (B,Ci,H,W), w (Ci*mult,1,k,k), b (Ci*mult) integer tensors -> y (B,Ci*mult,Ho,Wo) int64, from the definition, one shifted slice per tap:
    y[b][co][oy][ox] = bias[co] + sum_ky,kx w[co][ky][kx] x[b][co // mult][oy s - pad + ky][ox s - pad + kx], x = 0 outside the map"""
    x, w, b = x.to(torch.int64), w.to(torch.int64), b.to(torch.int64)
    B, Ci, H, W = x.shape
    Co, pad = Ci * mult, k // 2
    assert w.shape == (Co, 1, k, k) and b.shape == (Co,)
    Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
    xe = x.repeat_interleave(mult, dim=1) if mult > 1 else x
    y = b.view(1, Co, 1, 1).expand(B, Co, Ho, Wo).clone()
    for ky in range(k):
        oy0 = max(0, -((ky - pad) // stride))                    # first oy with oy s - pad + ky >= 0
        oy1 = min(Ho - 1, (H - 1 + pad - ky) // stride)          # last oy with oy s - pad + ky <= H - 1
        if oy1 < oy0:
            continue
        iy0 = oy0 * stride - pad + ky
        for kx in range(k):
            ox0 = max(0, -((kx - pad) // stride))
            ox1 = min(Wo - 1, (W - 1 + pad - kx) // stride)
            if ox1 < ox0:
                continue
            ix0 = ox0 * stride - pad + kx
            xs = xe[:, :, iy0:iy0 + (oy1 - oy0) * stride + 1:stride, ix0:ix0 + (ox1 - ox0) * stride + 1:stride]
            y[:, :, oy0:oy1 + 1, ox0:ox1 + 1] += xs * w[:, 0, ky, kx].view(1, Co, 1, 1)
    return y


def conv_f64(x, w, b, k, stride, mult):
    """the same convolution in float64 on the stored values (torch's conv2d)"""
    return F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=k // 2, groups=x.shape[1])


def conv_abs(x, w, b, k, stride, mult):
    """A = sum |w x| + |b| per output (float64): the magnitude the rounding bound of the Gaussian class scales with"""
    return conv_f64(x.double().abs(), w.double().abs(), b.double().abs(), k, stride, mult)


def gelu_erf(x):
    """the exact GELU x Phi(x) in float64"""
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ------------------------------------------------------------------------------------------------ GELU: the error each route's function is documented with
# max |error| against the erf form over all x, as the comments in csrc/common.h state them; test_gelu_emulations_hold_their_documented_error evaluates a float32
# emulation of both on a grid.  The Gaussian GELU bound reads E from here and from nowhere else.  (gelu_f's comment used to say 2.5e-5: the emulation measures
# 2.556e-5 at x = 3.081, so the comment and this table now say 2.6e-5; gelu2_n measures 4.92e-5 against its documented 5.1e-5)
GELU_ERR = {"gelu_f": 2.6e-5, "gelu2_n": 5.1e-5}
GELU_SLOPE = 1.13             # max |gelu'| = 1.1290 (at x = sqrt 2): what an error of the pre-activation grows to
_LOG2E = 1.4426950408889634


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def gelu_f_emulated(x):
    """float32 emulation of gelu_f (csrc/common.h): x * 1 / (1 + exp2(xc (a + b xc^2 + c xc^4))), xc = clamp(x, -8, 8); the hardware's exp2 / rcp are 1-ulp
    approximations, torch's are correctly rounded -- the difference is two float32 ulps of the result"""
    x = x.to(torch.float32)
    xc = x.clamp(-8.0, 8.0)
    x2 = xc * xc
    t = _f32(1.0142648e-3) * x2 - _f32(1.0677576e-1)
    t = t * x2 - _f32(2.3011213)
    e = torch.exp2(xc * t)
    return x * (1.0 / (1.0 + e))


GELU2_COEF = [0.398636314, -0.0658484117, 0.00950338221, -0.00101413109, 7.77420515e-05, -4.11762334e-06, 1.4164305e-07, -2.82720812e-09, 2.47331455e-11]


def _fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64"""
    return (a.double() * b.double() + c.double()).to(torch.float32)


def gelu2_n_emulated(x):
    """float32 emulation of gelu2_n (csrc/common.h): x * clamp(0.5 + xc P(xc^2), 0, 1), xc = clamp(x, -4.625, 4.625), P of degree 8 by Horner in fused
    multiply-adds"""
    x = x.to(torch.float32)
    xc = x.clamp(-4.625, 4.625)
    x2 = xc * xc
    c = [_f32(v) for v in GELU2_COEF]
    p = _fma32(x2, c[8], c[7])
    for i in range(6, -1, -1):
        p = _fma32(p, x2, c[i])
    phi = _fma32(xc, p, _f32(0.5)).clamp(0.0, 1.0)
    return x * phi


GELU_EMULATED = {"gelu_f": gelu_f_emulated, "gelu2_n": gelu2_n_emulated}


def gelu_of(kernel):
    """the GELU function a kernel calls when its gelu flag is set (None: the entry point has no flag)"""
    if kernel.startswith("dwpair"):
        return None
    return "gelu2_n" if kernel.startswith("dwconv_s2_mfma") else "gelu_f"


# ------------------------------------------------------------------------------------------------ the launchers' selection, restated
def dwconv_route(B, H, W, C, k, stride, mult):
    """launch_dwconv: {"kernel", "blocks", ...} or None where the launcher refuses"""
    if B <= 0 or H <= 0 or W <= 0 or C <= 0 or (C * mult) % 8:
        return None
    Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
    if stride == 1 and mult == 1 and k in (3, 7) and W >= 32 and C % 32 == 0:
        tiles_x, tiles_y, nsl = (W + 31) // 32, (H + 7) // 8, C // 32
        return {"kernel": f"dwconv_tile_kernel<{k}>", "blocks": B * tiles_x * tiles_y * nsl, "tiles_x": tiles_x, "tiles_y": tiles_y, "nsl": nsl, "tw": 32, "th": 8}
    if (k, stride, mult) not in INSTANCES:
        return None
    G, WQ = C * mult // 8, (Wo + 3) // 4
    GS = max(d for d in range(1, 17) if G % d == 0)
    nslices, qpb, nquads = G // GS, 256 // GS, B * Ho * WQ
    return {"kernel": f"dwconv_kernel<{k},{stride},{mult}>", "blocks": (nquads + qpb - 1) // qpb * nslices, "GS": GS, "nslices": nslices, "qpb": qpb,
            "idle": 256 - qpb * GS, "nquads": nquads, "last_quad": Wo % 4}


def dwconv_mfma_route(B, H, W, C, k):
    """launch_dwconv_mfma: {"kernel", "blocks", ...} or None where the launcher refuses"""
    if B <= 0 or H <= 0 or k not in (3, 7) or W < 16 or C % 32 or C <= 0:
        return None
    tiles_x, nsl = (W + 31) // 32, C // 32
    if k == 7 and H >= 16:
        return {"kernel": "dwconv_march_kernel<7>", "blocks": B * tiles_x * nsl, "tiles_x": tiles_x, "nsl": nsl, "groups": (H + 7) // 8, "tw": 32}
    th = 8                                                       # DW_TH7 is 8: the 16-row tile is compiled and never chosen
    tiles_y = (H + th - 1) // th
    return {"kernel": f"dwconv_mfma_kernel<{k},{th}>", "blocks": B * tiles_x * tiles_y * nsl, "tiles_x": tiles_x, "tiles_y": tiles_y, "nsl": nsl, "tw": 32, "th": th}


def dwconv_s2_route(B, H, W, C, cus):
    """launch_dwconv_s2_mfma on a device of `cus` compute units: {"kernel", "chains", "tpx", ...} or None where the launcher refuses"""
    if B <= 0 or H <= 0 or C <= 0 or C % 32 or H % 2 or W % 2 or W < 16:
        return None
    if cus <= 0:
        cus = 256
    Ho, Wo = H // 2, W // 2
    tiles_x, tiles_y, nsl = (Wo + 15) // 16, (Ho + 7) // 8, C // 32
    tiles = B * tiles_x * tiles_y
    tpx = (tiles + 7) // 8
    chains = max(1, (2 * cus // 8) // nsl)
    chains = min(chains, tpx)
    return {"kernel": "dwconv_s2_mfma_kernel", "chains": chains, "tpx": tpx, "tiles": tiles, "tiles_x": tiles_x, "tiles_y": tiles_y, "nsl": nsl,
            "blocks": 8 * chains * nsl, "tw": 16, "th": 8}


def dwconv_s2_walks(B, H, W, C, cus):
    """the persistent walk of dwconv_s2_mfma_kernel: for every (XCD, chain) of one channel slice, the list of (tile, image) the block visits, in order.  XCD x owns
    tiles [x tpx, min((x + 1) tpx, tiles)); chain c starts at x tpx + c and steps by `chains`"""
    r = dwconv_s2_route(B, H, W, C, cus)
    per_image = r["tiles_x"] * r["tiles_y"]
    walks = {}
    for xcd in range(8):
        t_end = min((xcd + 1) * r["tpx"], r["tiles"])
        for chain in range(r["chains"]):
            walks[(xcd, chain)] = [(t, t // per_image) for t in range(xcd * r["tpx"] + chain, t_end, r["chains"])]
    return walks


def dwconv_s2_walk_properties(B, H, W, C, cus):
    """what the walking case must have: (longest walk, some block's consecutive tiles lie in different images, the last XCD's range is shorter than tpx,
    every tile visited exactly once)"""
    r = dwconv_s2_route(B, H, W, C, cus)
    walks = dwconv_s2_walks(B, H, W, C, cus)
    longest = max(len(v) for v in walks.values())
    crosses = any(a[1] != b[1] for v in walks.values() for a, b in zip(v, v[1:]))
    last = min(8 * r["tpx"], r["tiles"]) - 7 * r["tpx"]
    visited = sorted(t for v in walks.values() for (t, _) in v)
    return {"longest": longest, "crosses_images": crosses, "last_xcd_short": r["tiles"] % 8 != 0 and last < r["tpx"], "complete": visited == list(range(r["tiles"]))}


def dwconv_pair_route(B, H, W, C):
    """launch_dwconv_pair: {"kernel", "geometry": (channels, columns) per block, "nstrips", "nseg", "starts": first group of every segment, ...} or None"""
    if B <= 0 or H < 16 or W < 32 or C <= 0 or C % 32 or (B * H + 16) * W * C * 2 > 0x7FFFFFF0:
        return None
    chb, tw = (64, 16) if C % 64 == 0 else (32, 32)              # DP_DEFAULT_GEO = 1, and geometry 0 where C % 64 != 0
    tiles_x, nsl = (W + tw - 1) // tw, C // chb
    nstrips = B * tiles_x * nsl
    ng, nseg = (H + 7) // 8, 1
    if nstrips < 256:
        nseg = max(1, min((512 + nstrips - 1) // nstrips, ng // 2))
    return {"kernel": f"dwpair_march_kernel<{chb},{tw}>", "geometry": (chb, tw), "nstrips": nstrips, "nseg": nseg, "blocks": nstrips * nseg, "groups": ng,
            "cut_to_half": nstrips < 256 and (512 + nstrips - 1) // nstrips > ng // 2 >= 1, "starts": [s * ng // nseg for s in range(nseg)], "tiles_x": tiles_x,
            "nsl": nsl, "tw": tw}


# ------------------------------------------------------------------------------------------------ instances
REACHABLE = (["dwconv_tile_kernel<3>", "dwconv_tile_kernel<7>"] + [f"dwconv_kernel<{k},{s},{m}>" for (k, s, m) in INSTANCES]
             + ["dwconv_march_kernel<7>", "dwconv_mfma_kernel<7,8>", "dwconv_mfma_kernel<3,8>", "dwconv_s2_mfma_kernel", "dwpair_march_kernel<64,16>",
                "dwpair_march_kernel<32,32>"])
# compiled into the product library and reached by no shape, with the reason
UNREACHABLE = {
    "dwconv_mfma_kernel<7,16>": "DW_TH7 is 8, and a 7x7 map with H >= 16 takes the march before the tile height is looked at",
    "dwconv_march_kernel<3>": "launched only under -DDW_MARCH3",
    "dwpair_march_kernel<32,16>": "geometry 2: DP_DEFAULT_GEO is 1, which falls back to geometry 0 and never to 2",
    "dwpair_march_kernel<64,8>": "geometry 3: DP_DEFAULT_GEO is 1",
}

# ------------------------------------------------------------------------------------------------ case tables (B = 2 unless the case says otherwise)
# VALU: (k, stride, mult, Ci, H, W).  Ci gives C mult / 8 = 1, 3, 17 (prime: GS = 1, 17 slices, 256 one-group quads per block) and 20 (GS = 10, 25 quads per
# block, 6 idle threads), doubled under mult 2 (2, 6, 34 -> GS 2, 40 -> GS 10).  (5, 3) is narrower than the window; every Wo here has Wo % 4 != 0 (17, 3, 7)
VALU_MAPS = {1: [(11, 17), (5, 3)], 2: [(9, 14), (10, 13)]}
VALU_CASES = [(k, s, m, Ci, H, W) for (k, s, m) in INSTANCES for Ci in (8, 24, 136, 160) for (H, W) in VALU_MAPS[s]]
# LDS-tiled VALU kernel: (k, C, H, W): one tile; a ragged last tile in both directions (19 = 2 x 8 + 3, 33 = 32 + 1); three column tiles, three slices
TILE_CASES = [(k, C, H, W) for k in (3, 7) for (C, H, W) in [(32, 8, 32), (64, 19, 33), (96, 9, 70)]]
# fv_op_dwconv_mfma: (kernel, k, C, H, W)
MFMA_CASES = ([("dwconv_mfma_kernel<7,8>", 7, C, H, W) for (C, H, W) in [(32, 8, 32), (64, 15, 37), (32, 9, 16), (64, 12, 20)]]       # the last two: half-masked strips
              + [("dwconv_mfma_kernel<3,8>", 3, C, H, W) for (C, H, W) in [(32, 16, 20), (96, 17, 40), (64, 33, 47), (32, 12, 16)]]
              + [("dwconv_march_kernel<7>", 7, C, H, W) for (C, H, W) in [(32, 16, 16), (64, 19, 33), (32, 24, 70), (96, 41, 32)]])   # the last: six groups, the ring wraps twice, the last group has one row
# fv_op_dwconv_s2_mfma: (C, H, W, B): smaller than one tile; ragged Ho % 8 and Wo % 16; 3 x 2 tiles, three slices; the walking case
S2_WALK_CASE = (1024, 50, 92, 3)      # nsl = 32 -> 2 chains at 256 CUs; Ho x Wo = 25 x 46: 4 x 3 tiles an image, 36 in all, tpx = 5; 27.6 MB of input
S2_CASES = [(32, 2, 16, 2), (64, 18, 34, 2), (96, 40, 64, 2), S2_WALK_CASE]
# fv_op_dwconv_pair: (kernel, C, H, W, B, nseg).  nseg = min(ceil(512 / nstrips), groups / 2) while nstrips < 256 -- with two or three row groups that is ONE
# segment (16 x 32, 19 x 37), 40 and 33 rows are cut to 5 / 2 = 2, 50 rows to 7 / 2 = 3 (starts 0, 2, 4: a segment of three groups).  The last two walk uncut
# over four units with 256 / 258 strips, the smallest B that gives 256
PAIR_CASES = [("dwpair_march_kernel<32,32>", 32, 16, 32, 2, 1), ("dwpair_march_kernel<32,32>", 96, 40, 64, 2, 2),
              ("dwpair_march_kernel<64,16>", 64, 19, 37, 2, 1), ("dwpair_march_kernel<64,16>", 128, 33, 50, 2, 2), ("dwpair_march_kernel<64,16>", 384, 16, 32, 2, 1),
              ("dwpair_march_kernel<64,16>", 64, 50, 37, 2, 3),
              ("dwpair_march_kernel<64,16>", 256, 32, 64, 16, 1), ("dwpair_march_kernel<32,32>", 96, 32, 64, 43, 1)]
PAIR_UNCUT = [c for c in PAIR_CASES if c[4] > 2]

# refusals: arguments of the entry point, each refused before anything is enqueued
DWCONV_REFUSED = [(2, 9, 14, 12, 3, 1, 1), (2, 9, 14, 8, 5, 1, 1), (2, 9, 14, 8, 7, 2, 1)]        # (B, H, W, C, k, stride, mult): (C mult) % 8, no such instance (twice)
MFMA_REFUSED = [(2, 16, 8, 32, 7), (2, 16, 16, 40, 7), (2, 16, 16, 32, 5)]                        # (B, H, W, C, k): W = 8, C = 40, k = 5
S2_REFUSED = [(2, 17, 16, 32), (2, 16, 14, 32), (2, 16, 16, 48)]                                  # (B, H, W, C): odd H, W = 14, C = 48
PAIR_REFUSED = [(2, 8, 32, 32), (2, 16, 16, 32), (2, 16, 32, 48)]                                 # (B, H, W, C): H = 8, W = 16, C = 48


# ------------------------------------------------------------------------------------------------ inputs
def gen(*key):
    s = 0
    for v in key:
        s = (s * 1000003 + int(v) + 12345) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g)


# exact class: (|x| max, |tap| max, |bias| max) by window
EXACT_RANGES = {7: (2, 1, 8), 3: (8, 3, 8)}
PAIR_TAPS7 = 20                       # non-zero (+-1) taps of the pair's 7x7 per channel
EXACT_LIMIT = 256                     # integers up to 2^8 are bf16 values


def exact_budget(k):
    """largest |output| the exact class can produce for a k x k window: every tap at its extreme"""
    xm, wm, bm = EXACT_RANGES[k]
    return k * k * xm * wm + bm


def exact_budget_pair():
    """(max |x'|, max |t|): x and the 3x3 taps in {-1, 0, 1}, |b3| <= 2; PAIR_TAPS7 taps of +-1 on x', |b7| <= 8"""
    xp = 9 * 1 * 1 + 2
    return xp, PAIR_TAPS7 * xp + 8


def exact_inputs(B, Ci, H, W, k, stride, mult, *key):
    """(x, w, b) int64: x (B,Ci,H,W), w (Ci mult,1,k,k), b (Ci mult) in the ranges of EXACT_RANGES[k]"""
    g = gen(B, Ci, H, W, k, stride, mult, 1, *key)
    xm, wm, bm = EXACT_RANGES[k]
    Co = Ci * mult
    return _ints((B, Ci, H, W), -xm, xm, g), _ints((Co, 1, k, k), -wm, wm, g), _ints((Co,), -bm, bm, g)


def exact_inputs_pair(B, C, H, W, *key):
    """(x, w3, b3, w7, b7) int64: x, w3 in {-1, 0, 1}; b3 in {-2, -1, 1, 2} (NON-ZERO: an x' "outside the map" that holds the 3x3's bias instead of the 7x7's zero
    padding changes t); w7 has exactly PAIR_TAPS7 taps of +-1 per channel; b7 in [-8, 8]"""
    g = gen(B, C, H, W, 37, *key)
    x, w3 = _ints((B, C, H, W), -1, 1, g), _ints((C, 1, 3, 3), -1, 1, g)
    b3 = _ints((C,), 1, 2, g) * (2 * _ints((C,), 0, 1, g) - 1)
    order = torch.rand(C, 49, generator=g).argsort(dim=1)
    w7 = torch.where(order < PAIR_TAPS7, 2 * _ints((C, 49), 0, 1, g) - 1, torch.zeros(C, 49, dtype=torch.int64)).view(C, 1, 7, 7)
    return x, w3, b3, w7, _ints((C,), -8, 8, g)


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def bf16_truncate(t):
    """fp32 -> the bf16 value below it in magnitude (the low 16 bits dropped): what a missing round-to-nearest does"""
    return (t.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32)


def gauss_inputs(B, Ci, H, W, k, stride, mult, *key, table):
    """the suite's recipe (tests/test_gpu_ops.py): x = bf16(randn), w = randn / k (bf16 values where the route reads a Toeplitz table, which stores bf16), b = 0.1 randn"""
    g = gen(B, Ci, H, W, k, stride, mult, 2, *key)
    Co = Ci * mult
    x = bf16_round(torch.randn(B, Ci, H, W, generator=g))
    w = torch.randn(Co, 1, k, k, generator=g) / k
    return x, (bf16_round(w) if table else w), torch.randn(Co, generator=g) * 0.1


# ------------------------------------------------------------------------------------------------ selection class
def selection_taps(Co, k):
    """channel c carries taps 1 + (ky k + kx) + (c % 5): every tap of a channel distinct, at most 53 (a bf16 value)"""
    return (1 + torch.arange(k * k).view(1, k * k) + (torch.arange(Co) % 5).view(Co, 1)).view(Co, 1, k, k).to(torch.int64)


def identity_taps(C, k):
    w = torch.zeros(C, 1, k, k, dtype=torch.int64)
    w[:, 0, k // 2, k // 2] = 1
    return w


def selection_positions(H, W, rows, cols):
    """the cross product of the interesting rows and columns that lie inside the map: the four corners, the last row and column, both sides of every boundary
    handed in, and one interior pixel.  Row and column 1 give the stride-2 maps an odd coordinate next to the border whatever the map's parity"""
    rs = sorted({r for r in [0, 1, H - 1, H // 2] + list(rows) if 0 <= r < H})
    cs = sorted({c for c in [0, 1, W - 1, W // 2] + list(cols) if 0 <= c < W})
    return [(r, c) for r in rs for c in cs]


def boundary_pairs(step, n, first=0, limit=None):
    """both sides of the boundaries first + step, first + 2 step, ... below n (at most `limit` of them)"""
    out, b = [], first + step
    while b < n and (limit is None or len(out) < 2 * limit):
        out += [b - 1, b]
        b += step
    return out


def pack_positions(positions, k):
    """impulse positions -> one list per batch entry, greedily, so that two impulses of one image are at least 2k apart (Chebyshev): their k x k patches cannot
    touch"""
    images = []
    for p in positions:
        for im in images:
            if all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 2 * k for q in im):
                im.append(p)
                break
        else:
            images.append([p])
    return images


def selection_input(images, C, H, W):
    """a single 1 at every position of every image's list, in every channel"""
    x = torch.zeros(len(images), C, H, W, dtype=torch.int64)
    for b, im in enumerate(images):
        for (r, c) in im:
            x[b, :, r, c] = 1
    return x


def selection_expected(images, w, H, W, k, stride, mult):
    """the mirrored tap patch stamped at every impulse and clipped to the map, written with explicit indices (independently of conv_int); also asserts that no two
    patches of one image overlap"""
    Co, pad = w.shape[0], k // 2
    Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
    y = torch.zeros(len(images), Co, Ho, Wo, dtype=torch.int64)
    hits = torch.zeros(len(images), Ho, Wo, dtype=torch.int64)
    for b, im in enumerate(images):
        for (r, c) in im:
            for ky in range(k):
                for kx in range(k):
                    ny, nx = r + pad - ky, c + pad - kx          # oy s - pad + ky = r
                    if ny % stride or nx % stride:
                        continue
                    oy, ox = ny // stride, nx // stride
                    if 0 <= oy < Ho and 0 <= ox < Wo:
                        y[b, :, oy, ox] += w[:, 0, ky, kx]
                        hits[b, oy, ox] += 1
    assert int(hits.max()) <= 1, "two impulses' patches overlap"
    return y


# ------------------------------------------------------------------------------------------------ the checks
def bits16(t):
    """a float tensor of bf16 values -> the bf16 bit patterns"""
    return t.to(torch.bfloat16).contiguous().view(torch.int16)


def check_exact(got, ref, what=""):
    """got: float tensor, ref: int64 -- equal as values, element for element (a -0 counts as 0)"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    g = got.double()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    bad = g != ref.double()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the integer reference, first at {tuple(int(v) for v in bad.nonzero()[0])}"


def check_bits(got, want, what=""):
    """bit for bit: the selection class (every expected value is a bf16 value; an unwritten or -0 element fails)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits16(got) != bits16(want.to(torch.float32))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ in their bits, first at {tuple(int(v) for v in bad.nonzero()[0])}"


def bf16_half_ulp(v):
    """half the spacing of the bf16 values around |v| (float64): 2^(floor(log2 |v|) - 8), 0 at 0.  bf16 keeps 8 significant bits, so this is 2^-9 of the TOP of
    v's binade: between 2^-9 |v| (just below a power of two) and 2^-8 |v| (at one).  Round-to-nearest never errs by more; truncation errs by up to twice as much"""
    v = v.double().abs()
    _, e = torch.frexp(v)                                        # v = m 2^e, m in [0.5, 1)
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), e - 9), torch.zeros_like(v))


def gauss_bound(pre, A, k, gelu=None, literal=False):
    """pre = the float64 convolution (before any GELU), A = sum |w x| + |b|.  delta = 2 k^2 2^-24 A covers the fp32 products' sum in any order, the bias add and
    the order inside an MFMA.  Returns (ref, bound):
      gelu None:  ref = pre,        |got - ref| <= hulp(|ref| + delta) + delta            one bf16 rounding of a value within delta of ref
      gelu name:  ref = gelu(pre),  the same with D = E + 1.13 delta in delta's place     E = GELU_ERR[name]; the pre-activation's delta grows by at most max |gelu'|
    hulp = bf16_half_ulp.  The rounding term is what tells rounding from truncation and is exactly what round-to-nearest can use up, no more.
    literal=True gives the form with 2^-9 (|ref| + D) in hulp's place, the relative half-ulp at the top of a binade only: a correctly rounded result reaches 1.98
    times that form just above a power of two (test_the_checks_tell_the_broken_arithmetics pins the figure), so it is reported and not asserted"""
    delta = 2.0 * k * k * 2.0 ** -24 * A
    if gelu is None:
        ref, D = pre, delta
    else:
        ref, D = gelu_erf(pre), GELU_ERR[gelu] + GELU_SLOPE * delta
    v = ref.abs() + D
    return ref, (2.0 ** -9 * v if literal else bf16_half_ulp(v)) + D


def gauss_fraction(got, pre, A, k, gelu=None, literal=False):
    """worst |got - ref| / bound over the tensor, and where"""
    ref, bound = gauss_bound(pre, A, k, gelu, literal)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    frac = (got.double() - ref).abs() / bound
    worst = float(frac.max())
    return worst, tuple(int(v) for v in (frac == frac.max()).nonzero()[0])


def check_gauss(got, pre, A, k, gelu=None, what=""):
    worst, where = gauss_fraction(got, pre, A, k, gelu)
    print(f"[dw-fwd gauss] {what}: worst |got - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: {worst:.3f} of the derived bound at {where}"
    return worst


# ------------------------------------------------------------------------------------------------ float32 / bf16 emulation, with defects to plant
def emulate_conv(x, w, b, k, stride, mult, *, gelu=None, truncate=False, zero_slot=None):
    """the kernels' arithmetic on the CPU: float32 products and sums (torch's conv2d in float32), the GELU emulation, one bf16 rounding.
    truncate: the output is truncated to bf16.  zero_slot = (channel, ky, kx, ox): the tap (ky, kx) of one channel is missing at ONE output column, which is what
    a zeroed slot of one strip column's Toeplitz fragment does"""
    C = x.shape[1]
    y = F.conv2d(x.float(), w.float(), b.float(), stride=stride, padding=k // 2, groups=C)
    if zero_slot is not None:
        co, ky, kx, ox = zero_slot
        pad = k // 2
        ix = ox * stride - pad + kx
        if 0 <= ix < x.shape[3]:
            for oy in range(y.shape[2]):
                iy = oy * stride - pad + ky
                if 0 <= iy < x.shape[2]:
                    y[:, co, oy, ox] -= w[co, 0, ky, kx].float() * x[:, co // mult, iy, ix].float()
    if gelu is not None:
        y = GELU_EMULATED[gelu](y)
    return bf16_truncate(y) if truncate else bf16_round(y)


def emulate_pair(x, w3, b3, w7, b7, *, unrounded=False, pad_b3=False, truncate=False):
    """x' = bf16(dw3x3(x) + b3), t = bf16(dw7x7(x') + b7) with x' = 0 outside the map.  unrounded: the 7x7 reads the float32 x' instead of the bf16 value that is
    stored.  pad_b3: x' outside the map is b3 (the 3x3's response to an empty window) instead of the 7x7's zero padding"""
    B, C, H, W = x.shape
    xp32 = F.conv2d(x.float(), w3.float(), b3.float(), padding=1, groups=C)
    xp = bf16_truncate(xp32) if truncate else bf16_round(xp32)
    src = xp32 if unrounded else xp
    if pad_b3:
        padded = b3.float().view(1, C, 1, 1).expand(B, C, H + 6, W + 6).clone()
        padded[:, :, 3:-3, 3:-3] = src
        t = F.conv2d(padded, w7.float(), b7.float(), padding=0, groups=C)
    else:
        t = F.conv2d(src, w7.float(), b7.float(), padding=3, groups=C)
    return xp, (bf16_truncate(t) if truncate else bf16_round(t))
