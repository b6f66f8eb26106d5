"""CPU-only helpers of the depthwise-backward op tests (tests/test_gpu_dw_backward.py, tests/test_dw_backward_reference_host.py): float64 autograd references, exact
int64 references, the Toeplitz table helpers, a mirror of the launchers' route selection, and the case tables both files read.

Layouts as the kernels take them: activations / gradients NHWC, taps tap-major [k*k][Ci*mult] with out-channel co = ci*mult + q.  The references work in NCHW
(torch's conv layout); nhwc() / nchw() convert.

The route mirror restates csrc/tower_bwd_kernels.hip (pick_slab, dw_bwd_scratch_floats, launch_dw_dgrad, launch_dw_wgrad) and csrc/tower_kernels.hip
(dw_dgrad_mfma_supported) for the PRODUCT build: the MFMA routes read their A/B environment switches once per process, the switches exist only in the tools build,
and the tests run with none set."""
import torch
import torch.nn.functional as F

INSTANCES = [(3, 1, 1), (7, 1, 1), (3, 2, 1), (7, 2, 2), (3, 1, 2)]   # (k, stride, mult) of every VALU kernel family
F16_MAX = 65504.0


def out_size(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def conv_weight(w, k, mult):
    """tap-major [k*k][Co] -> torch's grouped-conv weight (Co, 1, k, k); group ci owns out channels ci*mult .. ci*mult + mult - 1, the kernels' order"""
    return w.t().reshape(w.shape[1], 1, k, k).contiguous()


# ------------------------------------------------------------------------------------------------ float64 autograd references
def dgrad_ref(dy, w, res, Hi, Wi, k, stride, mult):
    """dy (B, Ci*mult, Ho, Wo), w tap-major [k*k][Ci*mult], res (B, Ci, Hi, Wi) or None -> dL/dx (B, Ci, Hi, Wi) in float64: torch.autograd over F.conv2d(groups=Ci)"""
    B, Co = dy.shape[0], dy.shape[1]
    Ci = Co // mult
    x = torch.zeros(B, Ci, Hi, Wi, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, conv_weight(w.double(), k, mult), None, stride=stride, padding=k // 2, groups=Ci)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    y.backward(dy.double())
    g = x.grad
    return g if res is None else g + res.double()


def wgrad_ref(x, dy, k, stride, mult):
    """x (B, Ci, Hi, Wi), dy (B, Ci*mult, Ho, Wo) -> (dw tap-major [k*k][Ci*mult], db [Ci*mult]) in float64: torch.autograd over F.conv2d(groups=Ci)"""
    Ci, Co = x.shape[1], dy.shape[1]
    assert Co == Ci * mult
    w = torch.zeros(Co, 1, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double(), w, b, stride=stride, padding=k // 2, groups=Ci)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    y.backward(dy.double())
    return w.grad.reshape(Co, k * k).t().contiguous(), b.grad


def dgrad_abs_ref(dy, w, Hi, Wi, k, stride, mult):
    """A = sum |w dy| per element of dx (float64): the magnitude the rounding bound of the Gaussian class scales with"""
    return dgrad_ref(dy.double().abs(), w.double().abs(), None, Hi, Wi, k, stride, mult)


# ------------------------------------------------------------------------------------------------ exact integer references
def _tap_ranges(n_in, n_out, k, stride, kk):
    """output positions o with 0 <= o*stride - pad + kk < n_in: (o0, o1, i0) with i = i0 + (o - o0) * stride; o1 exclusive"""
    pad = k // 2
    o0 = max(0, -((kk - pad) // stride))          # ceil((pad - kk) / stride)
    o1 = min(n_out - 1, (n_in - 1 + pad - kk) // stride)
    return o0, o1 + 1, o0 * stride - pad + kk


def dgrad_int(dy, w, res, Hi, Wi, k, stride, mult):
    """dgrad_ref on integer tensors, int64 throughout, written from the definition (one scatter per tap): dx[yi][xi] += w[ky][kx] dy[yo][xo], yi = yo s - pad + ky"""
    dy, w = dy.to(torch.int64), w.to(torch.int64)
    B, Co, Ho, Wo = dy.shape
    Ci = Co // mult
    dx = torch.zeros(B, Ci, Hi, Wi, dtype=torch.int64) if res is None else res.to(torch.int64).clone()
    for ky in range(k):
        y0, y1, iy0 = _tap_ranges(Hi, Ho, k, stride, ky)
        if y1 <= y0:
            continue
        for kx in range(k):
            x0, x1, ix0 = _tap_ranges(Wi, Wo, k, stride, kx)
            if x1 <= x0:
                continue
            term = (dy[:, :, y0:y1, x0:x1] * w[ky * k + kx].view(1, Co, 1, 1)).view(B, Ci, mult, y1 - y0, x1 - x0).sum(2)
            dx[:, :, iy0:iy0 + (y1 - y0 - 1) * stride + 1:stride, ix0:ix0 + (x1 - x0 - 1) * stride + 1:stride] += term
    return dx


def wgrad_int(x, dy, k, stride, mult):
    """wgrad_ref on integer tensors, int64 throughout: dw[ky k + kx][co] = sum dy[b][co][yo][xo] x[b][co // mult][yo s - pad + ky][xo s - pad + kx]"""
    x, dy = x.to(torch.int64), dy.to(torch.int64)
    B, Co, Ho, Wo = dy.shape
    Hi, Wi = x.shape[2], x.shape[3]
    xe = x.repeat_interleave(mult, dim=1)
    dw = torch.zeros(k * k, Co, dtype=torch.int64)
    for ky in range(k):
        y0, y1, iy0 = _tap_ranges(Hi, Ho, k, stride, ky)
        if y1 <= y0:
            continue
        for kx in range(k):
            x0, x1, ix0 = _tap_ranges(Wi, Wo, k, stride, kx)
            if x1 <= x0:
                continue
            xs = xe[:, :, iy0:iy0 + (y1 - y0 - 1) * stride + 1:stride, ix0:ix0 + (x1 - x0 - 1) * stride + 1:stride]
            dw[ky * k + kx] = (dy[:, :, y0:y1, x0:x1] * xs).sum((0, 2, 3))
    return dw, dy.sum((0, 2, 3))


# ------------------------------------------------------------------------------------------------ Toeplitz tables of the MFMA depthwise kernels
def toeplitz(w, k):
    """depthwise weights (C,1,k,k) -> table [C/16][k][NM][16][4 i][4 kk] = w[ky][4m + kk - i] (fastvla_hip.h; the forward stores it as bf16)."""
    Cc = w.shape[0]
    nm = (k + 6) // 4
    t = torch.zeros(Cc // 16, k, nm, 16, 4, 4)
    wv = w.view(Cc // 16, 16, k, k)
    for m in range(nm):
        for i in range(4):
            for kk in range(4):
                kx = 4 * m + kk - i
                if 0 <= kx < k:
                    t[:, :, m, :, i, kk] = wv[:, :, :, kx].permute(0, 2, 1)
    return t


def toeplitz_flipped16(w, k, flip=True):
    """tap-major [k*k][C] -> the fp16 table launch_dw_dgrad_mfma takes: the Toeplitz table of the FLIPPED taps (tap t takes tap k*k-1-t, toeplitz_flipped in
    csrc/tower_train.inc).  flip=False builds the unflipped table (what a forgotten flip would hand the kernel: the tests use it to show they would notice)."""
    wf = torch.flip(w, dims=[0]) if flip else w
    return toeplitz(conv_weight(wf.float(), k, 1), k).to(torch.float16)


# ------------------------------------------------------------------------------------------------ the launchers' selection, restated
def pick_slab(C, cap):
    best = 8
    for d in range(8, min(cap, C) + 1, 8):
        if C % d == 0:
            best = d
    return best


def _row_blocks(nrows, NPS, nslabs):
    return max(1, min(nrows // NPS, 3072 // nslabs))


def _lds_blocks(B, Ho, CS, nslabs):
    """(nb, gpb, gpi, ngroups) of launch_dw_wgrad's LDS-staged form"""
    NPS = 256 // (CS // 2)
    gpi = (Ho + NPS - 1) // NPS
    ngroups = B * gpi
    nb = min(max(512 // nslabs, 1), ngroups)
    gpb = (ngroups + nb - 1) // nb
    return (ngroups + gpb - 1) // gpb, gpb, gpi, ngroups


def wgrad_scratch_floats(B, Ho, Wo, Co, k):
    """dw_bwd_scratch_floats: partial-sum rows of (k*k + 1) * Co floats, enough for whichever route launch_dw_wgrad takes"""
    npb = min(512, (B * Ho * Wo + 255) // 256)
    CS = pick_slab(Co, 128)
    nslabs = Co // CS
    nrb = _row_blocks(B * Ho, 256 // (CS // 2), nslabs) + 1
    nlds = _lds_blocks(B, Ho, CS, nslabs)[0]
    return max(npb, nrb, nlds) * (k * k + 1) * Co


def dgrad_geometry(Ci, mult):
    """slab logic of launch_dw_dgrad: channels per slab, slabs, 8-channel groups per pixel, pixels per block, idle threads per block"""
    CS = pick_slab(Ci, 128 if mult == 1 else 64)
    G = CS // 8
    ppb = 256 // G
    return {"CS": CS, "nslabs": Ci // CS, "G": G, "ppb": ppb, "idle": 256 - ppb * G}


def dgrad_route(B, Hi, Wi, Ci, k, stride, mult):
    """launch_dw_dgrad: the kernel name, or None where the launcher refuses"""
    if B <= 0 or Hi <= 0 or Wi <= 0 or Ci <= 0 or Ci % 8 or (k, stride, mult) not in INSTANCES:
        return None
    return f"dw_dgrad_kernel<{k},{stride},{mult}>"


def dgrad_mfma_route(B, H, W, C, k):
    """launch_dw_dgrad_mfma (dw_dgrad_mfma_supported): the kernel name, or None where the launcher refuses"""
    if B <= 0 or C <= 0 or k not in (3, 7) or W < 16 or H < 16 or C % 32:
        return None
    return f"dwconv_march_kernel<{k},GRAD>"


def tower_dgrad_route(B, Hi, Wi, Ci, k, stride, mult):
    """dw_backward's choice in csrc/tower_train.inc: the MFMA route wherever a flipped table was built (stride 1, mult 1 and dw_dgrad_mfma_supported)"""
    if stride == 1 and mult == 1 and dgrad_mfma_route(B, Hi, Wi, Ci, k):
        return dgrad_mfma_route(B, Hi, Wi, Ci, k)
    return dgrad_route(B, Hi, Wi, Ci, k, stride, mult)


def wgrad_route(B, Hi, Wi, Ci, k, stride, mult):
    """launch_dw_wgrad: the kernel name, or None where the launcher refuses"""
    Co = Ci * mult
    if B <= 0 or Hi <= 0 or Wi <= 0 or Ci <= 0 or Co % 8 or (k, stride, mult) not in INSTANCES:
        return None
    Ho, Wo = out_size(Hi, k, stride), out_size(Wi, k, stride)
    CS = pick_slab(Co, 128)
    NT = k * k + 1
    inst = f"<{k},{stride},{mult}>"
    if k == 7 and stride == 1 and mult == 1 and Ci % 32 == 0 and Wi >= 32 and Hi >= 16 and B * ((Wi + 31) // 32) <= 512 and B * Hi * Wi * Ci * 2 < 1 << 40:
        nb = B * ((Wi + 31) // 32)
        if nb * (Ci // 32) <= 0x7fffffff and nb * NT * Co <= wgrad_scratch_floats(B, Ho, Wo, Co, k):
            return "dw_wgrad_mfma_kernel<7>"
    if Wo >= 8 and CS >= 32 * mult:
        NPS = 256 // (CS // 2)
        NR, NC = (NPS - 1) * stride + k, 7 * stride + k
        if NR * NC * (CS // mult // 8) <= 2560 and B * Hi * Wi * Ci * 2 < 0xfffffff0:
            return "dw_wgrad_lds_kernel" + inst
    if Wo >= 8:
        return "dw_wgrad_rows_kernel" + inst
    return "dw_wgrad_kernel" + inst


def wgrad_part_rows(B, Hi, Wi, Ci, k, stride, mult):
    """partial-sum rows the chosen route writes into scratch (each (k*k + 1) * Co floats): must fit wgrad_scratch_floats"""
    Co = Ci * mult
    Ho, Wo = out_size(Hi, k, stride), out_size(Wi, k, stride)
    CS = pick_slab(Co, 128)
    nslabs = Co // CS
    route = wgrad_route(B, Hi, Wi, Ci, k, stride, mult)
    if route.startswith("dw_wgrad_mfma"):
        return B * ((Wi + 31) // 32)
    if route.startswith("dw_wgrad_lds"):
        return _lds_blocks(B, Ho, CS, nslabs)[0]
    if route.startswith("dw_wgrad_rows"):
        nrows = B * Ho
        rpb = -(-nrows // _row_blocks(nrows, 256 // (CS // 2), nslabs))
        return -(-nrows // rpb)
    npix = B * Ho * Wo
    npb = min(512, (npix + 255) // 256)
    ppb = -(-npix // npb)
    return -(-npix // ppb)


# ------------------------------------------------------------------------------------------------ case tables (read by the GPU file and checked on the CPU)
# dgrad, VALU: (k, stride, mult, Ci, Hi, Wi).  Channel counts for the slab logic: 8 (one group per pixel), 24 (G = 3, ppb = 85, one idle thread), 96 (G = 12; with
# mult 2: slab 48, two slabs), 160 and 256 (two slabs).  Both maps of the instance's stride everywhere: (9, 14) / (10, 13) give both parities of the last row and
# column under stride 2 (some input positions receive no output), (11, 17) is neither a multiple of 8 nor of the pixels per block
_S1, _S2 = [(11, 17)], [(9, 14), (10, 13)]
DGRAD_CASES = [(k, s, m, Ci, Hi, Wi)
               for (k, s, m), chans in [((3, 1, 1), (8, 24, 160)), ((7, 1, 1), (24, 96, 256)), ((3, 2, 1), (8, 96, 160)), ((7, 2, 2), (24, 96)), ((3, 1, 2), (8, 96))]
               for Ci in chans for (Hi, Wi) in (_S2 if s == 2 else _S1)]
# dgrad, MFMA: (k, C, H, W): a half-masked strip; a second strip one column wide with H no multiple of 8; three slices; three strips; a ragged strip of the 3x3
DGRAD_MFMA_CASES = [(7, 32, 16, 16), (7, 64, 19, 33), (3, 96, 17, 40), (7, 32, 24, 70), (3, 32, 16, 20)]
DGRAD_MFMA_REFUSED = [(7, 32, 16, 8), (7, 40, 16, 16), (7, 32, 8, 16), (5, 32, 16, 16)]   # W = 8, C = 40, H = 8, k = 5
# wgrad: (route, k, stride, mult, Ci, Hi, Wi, B): one case at least per reachable (route x instance) pair; B in {1, 2, 3}
WGRAD_CASES = [
    ("dw_wgrad_mfma_kernel<7>", 7, 1, 1, 32, 19, 50, 2),
    ("dw_wgrad_mfma_kernel<7>", 7, 1, 1, 64, 16, 32, 3),
    ("dw_wgrad_lds_kernel<3,1,1>", 3, 1, 1, 32, 17, 33, 3),
    ("dw_wgrad_lds_kernel<7,1,1>", 7, 1, 1, 64, 16, 16, 2),
    ("dw_wgrad_lds_kernel<7,1,1>", 7, 1, 1, 48, 17, 33, 1),     # C % 32 != 0: off the matrix cores whatever the map
    ("dw_wgrad_lds_kernel<3,2,1>", 3, 2, 1, 64, 18, 34, 2),     # 4 blocks of partial sums where B * Ho / NPS + 1 is 3 (the scratch size found short)
    ("dw_wgrad_lds_kernel<7,2,2>", 7, 2, 2, 32, 17, 33, 2),
    ("dw_wgrad_lds_kernel<7,2,2>", 7, 2, 2, 96, 16, 32, 2),     # slab 96, two slabs
    ("dw_wgrad_lds_kernel<3,1,2>", 3, 1, 2, 48, 12, 20, 2),
    ("dw_wgrad_rows_kernel<3,1,1>", 3, 1, 1, 24, 12, 20, 2),
    ("dw_wgrad_rows_kernel<7,1,1>", 7, 1, 1, 24, 12, 20, 3),
    ("dw_wgrad_rows_kernel<3,2,1>", 3, 2, 1, 24, 18, 34, 2),
    ("dw_wgrad_rows_kernel<7,2,2>", 7, 2, 2, 24, 17, 33, 2),    # slab 48 < 64
    ("dw_wgrad_rows_kernel<3,1,2>", 3, 1, 2, 8, 12, 20, 1),
    ("dw_wgrad_kernel<3,1,1>", 3, 1, 1, 16, 10, 6, 2),          # Wo < 8 from here on
    ("dw_wgrad_kernel<7,1,1>", 7, 1, 1, 16, 10, 6, 2),
    ("dw_wgrad_kernel<3,2,1>", 3, 2, 1, 32, 9, 12, 2),
    ("dw_wgrad_kernel<7,2,2>", 7, 2, 2, 16, 9, 13, 3),
    ("dw_wgrad_kernel<3,1,2>", 3, 1, 2, 16, 9, 7, 1),
]
# every (route x instance) pair of the tap-gradient launcher and of the MFMA input gradient; the five VALU input-gradient instances are counted separately
# (DGRAD_CASES).  The issue that asked for these tests counts 17; written out it is 1 + 15 + 2 = 18 -- the cap on unreachable pairs (3) is what matters
ALL_PAIRS = (["dw_wgrad_mfma_kernel<7>"] + [f"{r}<{k},{s},{m}>" for r in ("dw_wgrad_lds_kernel", "dw_wgrad_rows_kernel", "dw_wgrad_kernel") for (k, s, m) in INSTANCES]
             + ["dwconv_march_kernel<3,GRAD>", "dwconv_march_kernel<7,GRAD>"])
# pairs no shape can reach, by name, with the condition that excludes them (none: every instance of every route has a shape of its own above)
UNREACHABLE = {}
MAX_UNREACHABLE = 3


def dgrad_bound(k, mult, with_res):
    """max |sum| of the exact class: taps in [-3, 3], dy in [-4, 4], res in [-512, 512]"""
    return k * k * mult * 3 * 4 + (512 if with_res else 0)


def wgrad_bound(B, Ho, Wo):
    """max |sum| of the exact class: x and dy in [-4, 4] over every output pixel"""
    return B * Ho * Wo * 4 * 4
