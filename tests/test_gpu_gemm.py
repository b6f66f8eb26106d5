"""-m gpu: launch_gemm (csrc/gemm_bf16.hip) at op level -- every kernel instance, tile walk, K-range form and reducer the product build can reach, each case
asserting the route the mirror (tests/gemm_util.py gemm_route) gives for THIS device's CU count, and that the library's own planner (fv_op_gemm_plan: plan_gemm,
which launch_gemm runs) gives the same route for the launch's arguments.

Three input classes (tests/gemm_util.py):
  exact      integer operands (split operands: hi integers, lo = j 2^-8) whose every partial sum fp32 holds exactly: fp32 outputs equal the float64 product bit
             for bit, bf16 / fp16 outputs its round-to-nearest-even; the K-range forms equal the call without scratch bit for bit
  selection  one-hot rows of A against W[n][k] = ((131 n + 71 k) mod 509) - 254: out[m][n] = W[n][pi(m)] bit for bit, every k-slot of both halves in turn
  Gaussian   per element against float64 on the stored values, bound D = (K_total + splits + 4) 2^-23 sum |a w| (+ a half-ulp of the output format), propagated
             through GELU / SwiGLU / the following RMSNorm; nothing here is tuned to a device result

Every launch writes into a NaN-filled output inside a larger allocation: sentinel elements before and behind every buffer, pad columns on lda / ldo / ldr, rows
past M and N of the operands holding +-1e4.  It must write every element, repeat its bits in a second run into fresh buffers, and leave guards, pads, operands,
bias, scale, residual and the memory around the scratch untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_util as G  # noqa: E402
from gemm_util import BIAS, F16, F32, RES_F32, SWIGLU_SPLIT, CASES, describe, route_key  # noqa: E402
from gpu_util import DEV, lib, stream  # noqa: E402

GUARD = 64              # sentinel elements before and behind every device buffer
EPS = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device (no CPU fallback in the product path)")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_route(c, epi, scratch=None, expect=None, bias=True):
    """the case's route on THIS device, by the mirror and by the library's own planner (fv_op_gemm_plan: plan_gemm, which launch_gemm runs) for the arguments the
    launch is about to get; a difference fails and names both"""
    cus = _cus()
    r = c.route(epi, cus, scratch=scratch, bias=bias)
    want = c.expect if expect is None else expect
    if route_key(r) != want:
        pytest.fail(f"{c.name} {G.EPI_NAME[epi]}: the case is there for {want} ({describe(c.route(epi, G.CUS, scratch=scratch))} at {G.CUS} CUs); "
                    f"this device has {cus} CUs and launch_gemm takes {describe(r)}")
    planned = G.library_route(lib(), **c.launch_args(epi, cus, scratch, bias))
    if planned != r:
        pytest.fail(f"{c.name} {G.EPI_NAME[epi]} at {cus} CUs: the library plans {describe(planned)} {planned}, the mirror says {describe(r)} {r}")
    return r


def _ibits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Buf:
    """a host tensor (or a fill value) inside a larger device allocation with GUARD sentinel elements on either side"""

    def __init__(self, host=None, shape=None, dtype=None, fill=float("nan")):
        shape = tuple(host.shape) if host is not None else tuple(shape)
        dtype = host.dtype if host is not None else dtype
        n = 1
        for s in shape:
            n *= s
        self.whole = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        if dtype == torch.uint8:
            self.whole.fill_(0x5a)
        else:
            self.whole.fill_(-7777.0)
        self.t = self.whole[GUARD:GUARD + n].view(shape)
        if host is not None:
            self.t.copy_(host)
        elif dtype == torch.uint8:
            self.t.fill_(int(fill))
        else:
            self.t.fill_(fill)
        self.before = self.whole.clone()

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return torch.equal(_ibits(self.whole[:GUARD]), _ibits(self.before[:GUARD])) and torch.equal(_ibits(self.whole[-GUARD:]), _ibits(self.before[-GUARD:]))

    def unchanged(self):
        return torch.equal(_ibits(self.whole), _ibits(self.before))


def _ptr(b):
    return None if b is None else b.ptr()


def _pack_w8(c, p):
    """the weights' fp8 copy as fv_op_lo8_pack stores it ([N][2K] bytes, the first K of a row valid); the reference reads the bytes back, so nothing depends on how
    the packer rounds"""
    w8 = Buf(shape=(c.N + G.GUARD_ROWS, 2 * c.K), dtype=torch.uint8, fill=0x7e)
    w = p.W.to(DEV).contiguous()
    rc = lib().fv_op_lo8_pack(None, None, 0, w.data_ptr(), w8.ptr(), c.M, c.K, c.N, stream())
    assert rc == 0, "fv_op_lo8_pack"
    torch.cuda.synchronize()
    assert w8.guards_intact()
    p.W8val = w8.t[:c.N, :c.K].contiguous().view(torch.float8_e4m3fn).float().cpu().double() / 64.0
    w8.before = w8.whole.clone()
    return w8


def launch(c, p, scratch=True, what=""):
    """one launch of problem p with every footprint check; returns the host outputs {"out": [M][ncols], "y", "ylo"}"""
    epi = p.epi
    ncols, ldo = c.ncols(epi), c.ldo(epi)
    A, W = Buf(p.A), Buf(p.W)
    bias = Buf(p.bias) if p.bias is not None else None
    scale = Buf(p.scale) if p.scale is not None else None
    res = Buf(p.res) if p.res is not None else None
    out = Buf(shape=(c.M, ldo), dtype=G.out_dtype(epi))
    nbytes = c.scratch if scratch else 0
    ws = Buf(shape=(nbytes // 4,), dtype=torch.float32) if nbytes else None
    w8 = _pack_w8(c, p) if c.ksplit == 2 else None
    normw = y = ylo = None
    if c.norm:
        if p.normw is None:
            p.normw = torch.ones(c.N)
        normw, y, ylo = Buf(p.normw), Buf(shape=(c.M, c.N + 8), dtype=torch.bfloat16), Buf(shape=(c.M, c.N + 8), dtype=torch.bfloat16)
    L, s = lib(), stream()
    if c.tn:
        rc = L.fv_op_gemm_tn(A.ptr(), c.lda, W.ptr(), c.ldw, c.M, c.N, c.K, int(c.f16), _ptr(bias), out.ptr(), ldo, _ptr(ws), nbytes, s)
    elif c.f16:
        rc = L.fv_op_gemm_f16(A.ptr(), c.lda, W.ptr(), c.M, c.N, c.K, _ptr(bias), _ptr(res), c.ldr() if res else 0, out.ptr(), ldo, epi, _ptr(ws), nbytes, s)
    elif c.ksplit == 2:
        rc = L.fv_op_gemm_lo8(A.ptr(), c.lda, W.ptr(), w8.ptr(), c.M, c.N, c.K, _ptr(bias), _ptr(res), c.ldr() if res else 0, out.ptr(), ldo, epi, _ptr(ws), nbytes, s)
    else:
        rc = L.fv_op_gemm_norm(A.ptr(), c.lda, W.ptr(), c.M, c.N, c.K, _ptr(bias), _ptr(scale), _ptr(res), c.ldr() if res else 0, out.ptr(), ldo, epi, c.ksplit,
                               _ptr(ws), nbytes, c.few_rows, _ptr(normw), _ptr(y), _ptr(ylo), c.N + 8 if c.norm else 0, EPS, s)
    assert rc == 0, f"{what}: launch_gemm returned {rc}: {L.fv_last_error(None)}"
    torch.cuda.synchronize()
    for name, b in (("A", A), ("W", W), ("bias", bias), ("scale", scale), ("residual", res), ("W8", w8), ("norm weight", normw)):
        assert b is None or b.unchanged(), f"{what}: {name} (or a sentinel around it) was written"
    for name, b in (("out", out), ("scratch", ws), ("y", y), ("y_lo", ylo)):
        assert b is None or b.guards_intact(), f"{what}: the sentinels around {name} were written"
    o = out.t.cpu()
    assert bool(torch.isnan(o[:, ncols if epi != SWIGLU_SPLIT else c.N:].float()).all()), f"{what}: ldo's pad columns were written"
    assert not bool(torch.isnan(o[:, :c.N if epi == SWIGLU_SPLIT else ncols].float()).any()), f"{what}: an element of the output was not written"
    got = {"out": o[:, :c.N if epi == SWIGLU_SPLIT else ncols].contiguous()}
    if c.norm:
        for k, b in (("y", y), ("ylo", ylo)):
            h = b.t.cpu()
            assert bool(torch.isnan(h[:, c.N:].float()).all()) and not bool(torch.isnan(h[:, :c.N].float()).any()), f"{what}: {k} not covered exactly"
            got[k] = h[:, :c.N].contiguous()
    return got


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(_ibits(a[k]), _ibits(b[k])), f"{what}: {k} differs between two runs"


def _twice(c, p, what):
    a, b = launch(c, p, what=what), launch(c, p, what=what + " (second run)")
    _same_bits(a, b, what)
    return a


FRACTIONS = {}          # case, epilogue -> worst fraction of the Gaussian bound


@pytest.fixture(scope="module", autouse=True)
def _print_the_worst_fractions():
    """after the file's last test: the per-case figures docs/kernels.md records (run with -s)"""
    yield
    for k in sorted(FRACTIONS):
        print(f"\n[gemm gauss worst] {k}: {FRACTIONS[k]:.3f}", end="")


def _note(c, epi, frac):
    k = f"{c.name} {G.EPI_NAME[epi]}"
    FRACTIONS[k] = max(FRACTIONS.get(k, 0.0), frac)


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("c", [c for c in CASES if c.epis], ids=repr)
def test_exact(c):
    """Integer operands inside the budget tests/test_gemm_reference_host.py asserts: fp32 outputs are the float64 product bit for bit, bf16 / fp16 outputs its
    round-to-nearest-even (most need rounding, some are ties); rows >= M and columns >= N of the operand buffers hold +-1e4 and must not reach a result; with
    scratch, the K-range form equals the one-pass call bit for bit; the RMSNorm outputs are checked against float64 on the returned rows."""
    for epi in c.epis:
        what = f"{c.name} {G.EPI_NAME[epi]} exact"
        _assert_route(c, epi)
        p = G.exact_problem(c, epi)
        got = _twice(c, p, what)
        G.check_bits(got["out"], G.exact_expected(p), what)
        if c.scratch:
            r1 = c.route(epi, _cus(), scratch=0)
            if isinstance(r1, list) or r1["splits"] != 1:
                pytest.fail(f"{what}: the call without scratch is meant to run in one pass; launch_gemm takes {describe(r1)}")
            one = launch(c, p, scratch=False, what=what + " (no scratch)")
            assert torch.equal(_ibits(one["out"]), _ibits(got["out"])), f"{what}: the K-range form differs from the call without scratch"
        if c.norm:
            G.norm_check(got["out"], got["y"], got["ylo"], p.normw, EPS, what)


# ------------------------------------------------------------------------------------------------ selection
def _selection_epi(c):
    for e in (F32, BIAS, RES_F32, F16):
        if e in c.epis:
            return e


@pytest.mark.parametrize("c", [c for c in CASES if c.epis], ids=repr)
def test_selection(c):
    """Row m of A is one-hot at k = pi(m); pi walks every k of both halves over the launches, a few rows select nothing.  The output is W[n][pi(m)] bit for bit (from
    the lo8 half: the weights' fp8 copy), +0 on the empty rows: every k-slot pairing of every fragment read -- the XOR swizzle, the TN transposing reads, the fp8
    32-byte operand, the zero-filled last K-tile at K % 64 != 0, the hi | lo seam."""
    epi = _selection_epi(c)
    _assert_route(c, epi, bias=False)
    for i in range(G.selection_launches(c)):
        what = f"{c.name} {G.EPI_NAME[epi]} selection launch {i}"
        p, pi = G.selection_problem(c, epi, i)
        got = _twice(c, p, what)
        if c.ksplit == 2:
            assert torch.equal(p.W8val, p.Wval), f"{what}: the weights' fp8 copy is not the weights (the class would not tell the lo8 half's k-slots apart)"
        G.check_bits(got["out"], G.selection_expected(p, pi), what)


# ------------------------------------------------------------------------------------------------ Gaussian
@pytest.mark.parametrize("c", [c for c in CASES if c.gauss], ids=repr)
def test_gauss(c):
    """x = 0.7 randn, W = randn / sqrt K, bias 0.1 randn, residual randn, rounded to the operand formats; every element (a column sample where the float64 product
    would take long) inside the bound derived in tests/gemm_util.py gauss_check; worst fractions measured on the MI355X: docs/kernels.md."""
    for epi in c.gauss:
        what = f"{c.name} {G.EPI_NAME[epi]} gauss"
        r = _assert_route(c, epi)
        p = G.gauss_problem(c, epi)
        got = _twice(c, p, what)          # the class where a summation order that varies from run to run shows: the exact class's sums have the same bits in any order
        cols = G.sample_cols(c, epi, r)
        o = got["out"]
        if epi == SWIGLU_SPLIT:
            I = c.N // 2
            hi, lo = o[:, :I], o[:, I:]
            if cols is not None:
                oc = G.out_cols(epi, cols)
                hi, lo = hi[:, oc], lo[:, oc]
            o = (hi, lo)
        elif cols is not None:
            o = o[:, G.out_cols(epi, cols)]
        _note(c, epi, G.gauss_check(p, o, G.splits_of(r), cols, what))
        if c.norm:
            G.norm_check(got["out"], got["y"], got["ylo"], p.normw, EPS, what)


def test_the_tail_against_the_one_pass_call_in_every_column():
    """(1024, 17408, 1024) with split operands: columns [0, 16384) run as they are, [16384, 17408) as a K-range problem of their own (RES_F32: test_exact[tail]
    compares every column bit for bit).  SwiGLU-split is no member of the exact class, but its accumulators are: with that class's integers both forms hand their
    epilogue the same fp32 gate and up.  Asserted: hi = bf16(silu_f(g) u) agrees bit for bit in all 8704 output columns, lo agrees bit for bit left of the cut
    (the same kernel in both calls), and right of it the two lo differ by no more than two evaluations of silu_f(g) u may: each is within SILU_ERR + SILU_REL
    (+ 2^-24 (1 + |g|): the product's rounding, and the exponent's argument g log2 e rounded at |g| beyond the range SILU_ERR was measured on) of the exact
    value, relative to it, and lo is rounded to bf16 once on either side.
    Measured on the MI355X: 6767 of the 524288 lo values right of the cut differ, by up to two fp32 ulps of o.  Bit equality is what one would want here and
    what the reducer's comment used to claim; it does not hold, nothing in the tree pins the cause, and which columns go to the reducer depends on the CU count:
    docs/kernels.md records it as an open point."""
    c = G.CASE["tail-swiglu"]
    r = _assert_route(c, SWIGLU_SPLIT)
    _assert_route(c, SWIGLU_SPLIT, scratch=0, expect=G.key("gemm256_kernel<8,4,ASYM>", "column-major"))
    p = G.exact_problem(G.CASE["tail"], RES_F32)
    p.epi, p.bias, p.res, p.c = SWIGLU_SPLIT, None, None, c
    a, b = launch(c, p, what="tail swiglu")["out"], launch(c, p, scratch=False, what="tail swiglu, no scratch")["out"]
    I, cut = c.N // 2, r[0]["cols"][1]
    assert torch.equal(_ibits(a[:, :I]), _ibits(b[:, :I])), "the hi halves differ"
    assert torch.equal(_ibits(a[:, I:I + cut // 2]), _ibits(b[:, I:I + cut // 2])), "the lo halves differ left of the cut, where both calls run the same kernel"
    gate, _ = G.swiglu_halves(G.reference(p, torch.arange(cut, c.N))[0])
    hi, la, lb = a[:, cut // 2:I].double(), a[:, I + cut // 2:].double(), b[:, I + cut // 2:].double()
    rel = 2 * (G.SILU_ERR + G.SILU_REL + 2.0 ** -24 * (1 + gate.abs()))
    hulp = G.bf16_half_ulp(torch.maximum(la.abs(), lb.abs())).clamp_min(2.0 ** -134)             # bf16's subnormal step is 2^-133
    bound = rel * (1 + 2.0 ** -8) * hi.abs() + 2.0 ** -149 + 2 * hulp
    frac = float(((la - lb).abs() / bound).max())
    print(f"[gemm tail] SwiGLU-split lo halves right of the cut: {int((la != lb).sum())} of {la.numel()} differ between the tail form and the one-pass call, "
          f"worst fraction of the bound {frac:.3f}")
    assert frac <= 1.0


# ------------------------------------------------------------------------------------------------ refusals
def _refusal_call(kw, misalign=0):
    """the launch gemm_route refuses, through the entry point that reaches it; returns (code, output unchanged)"""
    M, N, K = kw["M"], kw["N"], kw["K"]
    epi, ksplit, f16, tn, norm = kw["epi"], kw.get("ksplit", 0), kw.get("f16", False), kw.get("tn", False), kw.get("norm", False)
    lda, ldo = kw.get("lda", K), kw.get("ldo", N)
    dt = torch.float16 if f16 else torch.bfloat16
    A, W = Buf(shape=(256, 512), dtype=dt, fill=1.0), Buf(shape=(256, 512), dtype=dt, fill=1.0)
    odt = G.out_dtype(epi) if epi != 6 else torch.bfloat16
    out, res = Buf(shape=(256, 256), dtype=odt, fill=3.0), Buf(shape=(256, 256), dtype=torch.float32, fill=0.0)
    vec, y = Buf(shape=(512,), dtype=torch.float32, fill=1.0), Buf(shape=(256, 256), dtype=torch.bfloat16, fill=3.0)
    w8 = Buf(shape=(256, 1024), dtype=torch.uint8, fill=0)
    L, s = lib(), stream()
    a_ptr = A.ptr() + misalign
    if tn:
        rc = L.fv_op_gemm_tn(a_ptr, lda, W.ptr(), kw.get("ldw", N), M, N, K, int(f16), vec.ptr(), out.ptr(), ldo, None, 0, s)
    elif f16:
        rc = L.fv_op_gemm_f16(a_ptr, lda, W.ptr(), M, N, K, vec.ptr(), res.ptr(), N, out.ptr(), ldo, epi, None, 0, s)
    elif ksplit == 2:
        rc = L.fv_op_gemm_lo8(a_ptr, lda, W.ptr(), w8.ptr(), M, N, K, vec.ptr(), res.ptr(), N, out.ptr(), ldo, epi, None, 0, s)
    else:
        rc = L.fv_op_gemm_norm(a_ptr, lda, W.ptr(), M, N, K, vec.ptr(), vec.ptr(), res.ptr(), N, out.ptr(), ldo, epi, ksplit, None, 0, 1,
                               vec.ptr() if norm else None, y.ptr() if norm else None, None, N if norm else 0, EPS, s)
    torch.cuda.synchronize()
    return rc, out.unchanged() and y.unchanged()


@pytest.mark.parametrize("what,kw", G.REFUSED, ids=[w for w, _ in G.REFUSED])
def test_refusals_enqueue_nothing(what, kw):
    assert G.refused(G.gemm_route(**kw)), "the mirror admits it"
    rc, untouched = _refusal_call(kw)
    assert rc != 0, f"{what}: accepted"
    assert untouched, f"{what}: refused, but the output was written"


def test_a_misaligned_pointer_is_refused():
    kw = dict(M=64, N=64, K=64, lda=64, epi=BIAS)
    assert not G.refused(G.gemm_route(**kw))
    rc, untouched = _refusal_call(kw, misalign=8)
    assert rc != 0 and untouched
    rc, _ = _refusal_call(kw)
    assert rc == 0                                     # the same launch, aligned, is taken
