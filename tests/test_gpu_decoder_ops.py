"""-m gpu: the parity-mode decoder's HBM-bound forward kernels, each on its own against a float64 reference of the same operation
(csrc/decoder_kernels.hip, csrc/attention_split.hip, through the test-only entry points fv_op_attention_f32 / fv_op_rmsnorm_forms / fv_op_embed_gather /
fv_op_pool_norm of include/fastvla_hip_testops.h).

Attention ([site] transformers/models/qwen2/modeling_qwen2.py:105-135, 150-234).  The three routes of launch_attention_f32 -- the split-bf16 kernels, the
fp32-MFMA kernel (with its cached-prefix form, len_add, the hi + lo8 output and the row statistics) and the head_dim-32 VALU kernel with its in-place rotation --
at the smallest shapes that cross each tile edge (tests/attn_ref_util.py CASES).  Measure: the WORST QUERY ROW, max over (batch, head, t) of
||got - ref|| / ||ref|| over the head's D values, never a norm over the batch.  Bound: 2 x the worst row of the matching CPU emulation of the kernel's
arithmetic against the same float64 reference on the same inputs (the factor covers __expf / __logf and summation order; the emulations' own error is capped
in tests/test_attention_reference_host.py); lse the same in absolute error plus 2^-22 max(1, |lse|).  Output buffers carry a sentinel bit pattern in their
padding columns and one extra row, which must survive; where lens[b] < T only the rows < len are compared (rows past the prompt are never consumed).

Glue: every output form of rmsnorm_kernel, embed_gather_kernel (splice, id clamp) and pool_norm_kernel (both modes, Ni offset, len clamp), with bounds taken
from the number formats."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref_util as A  # noqa: E402
from gpu_util import DEV, call, lib, stream  # noqa: E402

SENT16 = 0x7FA5            # a bf16 / fp16 NaN pattern no kernel writes
SENT32 = 0x7FC5A5A5        # an fp32 NaN pattern


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device (no CPU fallback in the product path)")


def _sent16(rows, cols):
    return torch.full((rows, cols), SENT16, dtype=torch.int16, device=DEV)


def _sent32(n):
    return torch.full((n,), SENT32, dtype=torch.int32, device=DEV)


def _padded(t2d, ld, g):
    """(rows, w) fp32 -> device (rows, ld) with the data in the first w columns and other finite values in the padding"""
    rows, w = t2d.shape
    buf = torch.randn(rows, ld, generator=g) * 3.0
    buf[:, :w] = t2d
    return buf.to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------ attention
def _run_attention(c, qkv, pre, table, *, lens="case", use_split=None):
    """one fv_op_attention_f32 call at case c's settings -> dict of CPU tensors: o (B, Tq, heads, D) float64 decoded hi + lo, raw (rows + 1, ldo) int16 bits,
    lse (B, heads, T) or None with lse_raw int32 bits, qkv_after (B Tq, ld) and pre_after as the call left the inputs"""
    B, T, heads, kv, D, Np = c.B, c.T, c.heads, c.kv, c.D, c.Np
    Tq, qd, w = T - Np, heads * D, (heads + 2 * kv) * D
    ld, ldo, ldp = w + A.PAD, 2 * qd + A.PAD, 2 * kv * D + A.PAD
    g = torch.Generator().manual_seed(11)
    q_dev = _padded(qkv.reshape(B * Tq, w), ld, g)
    q_before = q_dev.clone()
    p_dev = _padded(pre.reshape(B * Np, 2 * kv * D), ldp, g) if Np else None
    p_before = p_dev.clone() if Np else None
    t_dev = table.to(DEV).contiguous() if table is not None else None
    if isinstance(lens, str):
        lens = c.lens
    l_dev = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    out = _sent16(B * Tq + 1, ldo)
    lse = _sent32(B * heads * T + 8) if c.lse else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    call(lib().fv_op_attention_f32(q_dev.data_ptr(), ld, out.data_ptr(), ldo, B, T, heads, kv, D, ptr(l_dev), c.len_add, ptr(t_dev), ptr(p_dev), ldp if Np else 0, Np,
                                   ptr(lse), int(c.lo8), int(c.use_split if use_split is None else use_split), stream()), f"fv_op_attention_f32 {c.name}")
    torch.cuda.synchronize()
    raw = out.cpu()
    # sentinels: the padding columns of every row, the extra row, and with lo8 the unused second half of the lo columns
    used = 2 * qd if not c.lo8 else qd + qd // 2
    assert bool((raw[:B * Tq, used:] == SENT16).all()), f"{c.name}: padding columns written"
    assert bool((raw[B * Tq] == SENT16).all()), f"{c.name}: a row past the output written"
    body = raw[:B * Tq]
    hi = body[:, :qd].contiguous().view(torch.bfloat16).float()
    if c.lo8:
        lo = body.contiguous().view(torch.uint8)[:, 2 * qd:3 * qd].contiguous().view(torch.float8_e4m3fn).float() / 256.0    # the bytes sit at the lo half's byte offset
    else:
        lo = body[:, qd:2 * qd].contiguous().view(torch.bfloat16).float()
    o = (hi.double() + lo.double()).view(B, Tq, heads, D)
    res = {"o": o, "raw": raw, "hi": hi, "lo": lo, "qkv_after": q_dev.cpu(), "qkv_before": q_before.cpu(), "lse": None}
    if Np:
        assert torch.equal(p_dev.cpu(), p_before.cpu()), f"{c.name}: the prefix cache was written"
    if c.lse:
        lraw = lse.cpu()
        assert bool((lraw[B * heads * T:] == SENT32).all()), f"{c.name}: lse written past its end"
        res["lse"] = lraw[:B * heads * T].view(torch.float32).view(B, heads, T).clone()
        res["lse_raw"] = lraw
    return res


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_attention_f32_worst_row_against_float64(name):
    """Every route and form at its case's shape: the worst query row and the worst lse against float64 within twice the emulation's own error; the inputs
    untouched (head_dim 64 / 128), or rotated in place exactly as rope_f32 rotates (head_dim 32); a second call bit-identical; and rows >= len of qkv
    rewritten with other finite values leave every row < len bit-identical (masked keys contribute exact zeros)."""
    r = A.reference(name)
    c = r["case"]
    got = _run_attention(c, r["qkv"], r["pre"], r["table"])
    ok = A.valid_rows(c)
    assert torch.isfinite(got["o"][ok]).all()
    worst, bound = A.worst_row(got["o"], r["o64"], c), 2.0 * r["emu_worst"]
    print(f"[{name}] route {c.route}: worst row {worst:.2e} (emulation {r['emu_worst']:.2e}, bound {bound:.2e})")
    assert r["emu_worst"] <= A.CAPS[c.form]
    assert worst <= bound, f"{name}: worst row {worst:.3e} > 2 x emulation {r['emu_worst']:.3e}"
    if c.lse:
        ref = r["lse64"].transpose(1, 2)[ok]                           # (valid rows, heads)
        err = (got["lse"].double().transpose(1, 2)[ok] - ref).abs()
        lim = 2.0 * r["emu_lse_err"] + 2.0 ** -22 * ref.abs().clamp_min(1.0)
        print(f"[{name}] lse: worst abs error {float(err.max()):.2e} (emulation {r['emu_lse_err']:.2e})")
        assert bool((err <= lim).all()), f"{name}: lse off by {float((err - lim).max()):.3e} beyond the bound"
    # the inputs
    qd, kd = c.heads * c.D, c.kv * c.D
    before, after = got["qkv_before"], got["qkv_after"]
    if c.D >= 64 or not c.rope:
        assert torch.equal(after, before), f"{name}: qkv was written"
    else:   # head_dim 32 with a table: q and k rotated in place, v and the padding untouched
        assert torch.equal(after[:, qd + kd:], before[:, qd + kd:])
        x = before[:, :qd + kd].double().reshape(c.B, c.T, c.heads + c.kv, c.D)
        want = A._rotate(x, r["table"], 0, torch.float64)
        h = c.D // 2
        mag = torch.cat([x[..., :h].abs() + x[..., h:].abs()] * 2, dim=-1)   # |a| + |b| >= |a cos| + |b sin|: two products and a sum, each rounded once
        d = (after[:, :qd + kd].double().reshape(want.shape) - want).abs()
        assert bool((d <= 3 * 2.0 ** -24 * mag).all()), f"{name}: in-place rotation off by {float(d.max()):.3e}"
    # a second identical call
    again = _run_attention(c, r["qkv"], r["pre"], r["table"])
    assert torch.equal(again["raw"], got["raw"]), f"{name}: two identical calls differ"
    if c.lse:
        assert torch.equal(again["lse_raw"], got["lse_raw"])
    # rows >= len rewritten
    klens = c.key_lens()
    if min(klens) < c.T:
        q2 = r["qkv"].clone()
        gg = torch.Generator().manual_seed(5)
        for b in range(c.B):
            n = max(klens[b] - c.Np, 0)
            q2[b, n:] = torch.randn(q2[b, n:].shape, generator=gg) * 5.0 + 1.0
        other = _run_attention(c, q2, r["pre"], r["table"])
        rows = ok.reshape(-1)
        assert torch.equal(other["raw"][:-1][rows], got["raw"][:-1][rows]), f"{name}: rows < len depend on rows >= len"
        if c.lse:
            assert torch.equal(other["lse"].transpose(1, 2)[ok], got["lse"].transpose(1, 2)[ok])


@pytest.mark.parametrize("name", [c.name for c in A.CASES if min(c.key_lens()) < c.T])
def test_attention_f32_rows_past_the_prompt_see_only_the_keys_below_len(name):
    """For a query i < len causality (j <= i) already implies j < len, so the key-length term of the mask acts ONLY on the query rows >= len.  The decoder never
    consumes those rows, but they are where `j < len` -- and with it lens + len_add and its clamp -- can be observed at all: a `<=` there, or a length taken
    without len_add, changes nothing else.  The kernels compute them (every query of a block attends to the keys j <= i, j < len), the oracle's mask defines
    them the same way (oracle/qwen2.py decoder_forward: causal & key_ok), so they are held to the same float64 reference under the same rule: the worst such
    row within twice the emulation's worst such row."""
    r = A.reference(name)
    c = r["case"]
    got = _run_attention(c, r["qkv"], r["pre"], r["table"])
    past = ~A.valid_rows(c)
    assert bool(past.any())
    emu = float(A.row_errors(r["emu"], r["o64"])[past].max())
    worst = float(A.row_errors(got["o"], r["o64"])[past].max())
    print(f"[{name}] rows >= len: worst row {worst:.2e} (emulation {emu:.2e})")
    assert emu <= A.CAPS[c.form]
    assert worst <= 2.0 * emu, f"{name}: worst row past the prompt {worst:.3e} > 2 x emulation {emu:.3e}"
    if c.lse:
        ref = r["lse64"].transpose(1, 2)[past]
        e_emu = float((r["emu_lse"].double().transpose(1, 2)[past] - ref).abs().max())
        err = (got["lse"].double().transpose(1, 2)[past] - ref).abs()
        assert bool((err <= 2.0 * e_emu + 2.0 ** -22 * ref.abs().clamp_min(1.0)).all()), f"{name}: lse past the prompt off by {float(err.max()):.3e}"


@pytest.mark.parametrize("name", [c.name for c in A.CASES if c.Np])
def test_attention_f32_prefix_equals_the_joint_call_bit_for_bit(name):
    """The cached-prefix form against ONE call over all T positions (no scratch: the same fp32-MFMA kernel), on the rows >= Np, bit for bit: key tiles are
    aligned to 16 from position 0 in both, every query meets the same visible keys in the same order, and a tile that is fully masked for a query (the two
    forms' waves start at other queries, so a query may sit in a wave that walks one more tile) multiplies its accumulators by exp(0) = 1 and adds zeros."""
    r = A.reference(name)
    c = r["case"]
    got = _run_attention(c, r["qkv"], r["pre"], r["table"])
    cj = A.Case(c.name + "_joint", c.B, c.T, c.heads, c.kv, c.D, lens=c.lens, len_add=c.len_add)
    joint = _run_attention(cj, r["full"], None, r["table"], use_split=0)
    qd = c.heads * c.D
    a = got["raw"][:-1, :2 * qd].view(c.B, c.T - c.Np, 2 * qd)
    b = joint["raw"][:-1, :2 * qd].view(c.B, c.T, 2 * qd)[:, c.Np:]
    assert torch.equal(a, b), f"{name}: {int((a != b).sum())} output halves differ from the joint call"


def test_attention_f32_wrapper_rejects_what_it_cannot_run():
    L = lib()
    buf = torch.zeros(64, 1024, device=DEV)
    out = torch.zeros(64, 1024, dtype=torch.bfloat16, device=DEV)
    assert L.fv_op_attention_f32(buf.data_ptr(), 1024, out.data_ptr(), 256, 1, 8, 4, 2, 64, None, 0, None, None, 0, 0, None, 0, 0, stream()) != 0   # ldo < 2 heads D
    assert L.fv_op_attention_f32(buf.data_ptr(), 1024, out.data_ptr(), 1024, 1, 8, 4, 2, 32, None, 0, None, None, 0, 0, None, 0, 1, stream()) != 0  # split at head_dim 32
    assert L.fv_op_attention_f32(buf.data_ptr(), 1024, out.data_ptr(), 1024, 1, 8, 4, 2, 48, None, 0, None, None, 0, 0, None, 0, 0, stream()) != 0  # head_dim
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------------------------- rmsnorm
def _rms_ref64(x, w, eps):
    x, w = x.double(), w.double()
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def _half_ulp_bf16(hi):
    """half a unit in the last place of a bf16 value (8 significant bits): hi = m 2^e, m in [0.5, 1) -> ulp = 2^(e - 8)"""
    _, e = torch.frexp(hi.double())
    return torch.ldexp(torch.ones_like(hi, dtype=torch.float64), e - 9)


def _rmsnorm_forms(x, w, *, form, eps=1e-6):
    """form "split" | "plain" | "lo8" | "f16" -> (raw (rows + 1, ldy) int16 CPU, sat count or None)"""
    rows, H = x.shape
    ldy = 2 * H + 16
    xd, wd = x.to(DEV).contiguous(), w.to(DEV).contiguous()
    y = _sent16(rows + 1, ldy)
    sat = torch.zeros(1, dtype=torch.int32, device=DEV) if form == "f16" else None
    y_lo = None if form in ("plain", "f16") else y.data_ptr() + 2 * H
    call(lib().fv_op_rmsnorm_forms(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), y_lo, ldy, rows, H, eps, int(form == "f16"), sat.data_ptr() if sat is not None else None,
                                   int(form == "lo8"), stream()), f"fv_op_rmsnorm_forms {form}")
    torch.cuda.synchronize()
    raw = y.cpu()
    used = {"split": 2 * H, "plain": H, "f16": H, "lo8": H + H // 2}[form]
    assert bool((raw[:rows, used:] == SENT16).all()) and bool((raw[rows] == SENT16).all()), f"rmsnorm {form}: sentinel columns / row written"
    return raw[:rows], (int(sat.item()) if sat is not None else None)


@pytest.mark.parametrize("rows", [1, 5, 37])
@pytest.mark.parametrize("H", [64, 520, 896, 3584])
def test_rmsnorm_output_forms(rows, H):
    """[site] modeling_qwen2.py:247-252.  H = 64: 8 of a wave's 64 lanes busy; 520: H % 512 != 0 (one lane makes a second trip); 3584: seven trips.
    split: |hi + lo - ref| <= 2^-16 |ref| (the format's 2^-17 plus fp32 arithmetic), |lo| <= half an ulp of hi; plain: hi is the split form's hi;
    lo8: <= 2^-13 |ref| + 2^-18 (three mantissa bits on a remainder of at most 2^-9, plus e4m3's subnormal step over 256);
    fp16: within fp16 rounding of the reference, and the saturation counter is 0."""
    g = torch.Generator().manual_seed(rows * 10000 + H)
    x = torch.randn(rows, H, generator=g) * (0.5 + 3.0 * torch.rand(rows, 1, generator=g))
    w = 1.0 + 0.3 * torch.randn(H, generator=g)
    ref = _rms_ref64(x, w, 1e-6)
    raw, _ = _rmsnorm_forms(x, w, form="split")
    hi, lo = raw[:, :H].contiguous().view(torch.bfloat16).double(), raw[:, H:2 * H].contiguous().view(torch.bfloat16).double()
    err = (hi + lo - ref).abs()
    print(f"[rmsnorm {rows}x{H}] split: max |hi + lo - ref| / |ref| {float((err / ref.abs()).max()):.2e} (bound {2.0 ** -16:.2e})")
    assert bool((err <= 2.0 ** -16 * ref.abs()).all()), f"split: {float((err / ref.abs()).max()):.3e}"
    assert bool((lo.abs() <= _half_ulp_bf16(hi)).all())
    plain, _ = _rmsnorm_forms(x, w, form="plain")
    assert torch.equal(plain[:, :H], raw[:, :H])
    raw8, _ = _rmsnorm_forms(x, w, form="lo8")
    assert torch.equal(raw8[:, :H], raw[:, :H])
    lo8 = raw8.contiguous().view(torch.uint8)[:, 2 * H:3 * H].contiguous().view(torch.float8_e4m3fn).double() / 256.0
    err8 = (hi + lo8 - ref).abs()
    print(f"[rmsnorm {rows}x{H}] lo8: max error / (2^-13 |ref| + 2^-18) {float((err8 / (2.0 ** -13 * ref.abs() + 2.0 ** -18)).max()):.2f}")
    assert bool((err8 <= 2.0 ** -13 * ref.abs() + 2.0 ** -18).all())
    raw16, sat = _rmsnorm_forms(x, w, form="f16")
    y16 = raw16[:, :H].contiguous().view(torch.float16).double()
    assert bool(((y16 - ref).abs() <= 2.0 ** -11 * (1 + 2.0 ** -10) * ref.abs() + 2.0 ** -25).all())   # round to nearest at 11 bits of an fp32 value 2^-21 off; fp16's subnormal step
    assert sat == 0


@pytest.mark.parametrize("rows,H", [(5, 64), (37, 520), (5, 896)])
def test_rmsnorm_f16_counts_saturated_groups(rows, H):
    """Weights of 3e5 on a few columns push their outputs past 65504 wherever |x rsqrt(..)| > 0.22: the counter must equal the number of 8-element GROUPS
    that hold a clamped value (it counts groups, not elements), those values must be exactly +-65504, and the rest are rounded as usual."""
    g = torch.Generator().manual_seed(rows + H)
    x = torch.randn(rows, H, generator=g)
    w = 1.0 + 0.3 * torch.randn(H, generator=g)
    big = [3, 4, 17, H - 1] + ([515] if H > 515 else [])     # two in one group, one alone, the last column, the second trip's only group
    w[big] = 3.0e5
    ref = _rms_ref64(x, w, 1e-6)
    over = ref.abs() > 65504.0
    assert not bool(((ref.abs() - 65504.0).abs() < 1.0).any())          # nothing near the threshold: the expected count is not a matter of rounding
    groups = int(over.view(rows, H // 8, 8).any(dim=-1).sum())
    assert 0 < groups < int(over.sum())                                  # so that counting elements would give another number
    raw16, sat = _rmsnorm_forms(x, w, form="f16")
    y16 = raw16[:, :H].contiguous().view(torch.float16).double()
    assert sat == groups, (sat, groups, int(over.sum()))
    assert torch.equal(y16[over], torch.sign(ref[over]) * 65504.0)
    assert bool(((y16 - ref).abs()[~over] <= (2.0 ** -11 * (1 + 2.0 ** -10) * ref.abs() + 2.0 ** -25)[~over]).all())


# --------------------------------------------------------------------------------------------------------------------------- embed gather
@pytest.mark.parametrize("Ni", [0, 5])
@pytest.mark.parametrize("H", [64, 520, 896])
def test_embed_gather_is_exact(Ni, H):
    """x rows = the image tokens, then table[id] widened to fp32, bit for bit; ids below 0 and >= vocab clamp to the ends; B (Ni + T) = 18 / 33 rows: the last
    block of four waves is ragged."""
    B, T, vocab = 3, 6, 50
    g = torch.Generator().manual_seed(Ni * 1000 + H)
    table = torch.randn(vocab, H, generator=g).to(torch.bfloat16)
    img = torch.randn(B, Ni, H, generator=g) if Ni else None
    ids = torch.randint(0, vocab, (B, T), generator=g, dtype=torch.int32)
    ids[0, 0], ids[0, 1], ids[1, 2], ids[2, 5], ids[2, 4], ids[1, 0] = -3, vocab + 5, -(2 ** 31), 2 ** 31 - 1, 0, vocab - 1
    rows = B * (Ni + T)
    assert rows % 4
    x = _sent32((rows + 1) * H).view(rows + 1, H)
    td, idd = table.to(DEV), ids.to(DEV)
    imd = img.to(DEV).contiguous() if Ni else None
    call(lib().fv_op_embed_gather(idd.data_ptr(), td.data_ptr(), imd.data_ptr() if Ni else None, x.data_ptr(), B, T, Ni, H, vocab, stream()), "fv_op_embed_gather")
    torch.cuda.synchronize()
    raw = x.cpu()
    assert bool((raw[rows] == SENT32).all())
    got = raw[:rows].view(torch.float32).view(B, Ni + T, H)
    want = table[ids.long().clamp(0, vocab - 1)].float()
    if Ni:
        want = torch.cat([img, want], dim=1)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------ pool norm
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Ni", [0, 5])
@pytest.mark.parametrize("H", [64, 100, 896])
def test_pool_norm_modes_offsets_and_clamps(mode, Ni, H):
    """reference model/fastvlm_adapter.py:337-359 as oracle/qwen2.py llm_pooled applies it: mode 0 = the final RMSNorm of row Ni + max(len - 1, 0), mode 1 = the
    mean of the normed rows 0 .. Ni + len - 1.  lens = T, 1, 0 (which clamps to row Ni), 3, T + 9 (clamps to T), and once lens = NULL.
    Bound, elementwise: 2 (R + 8) 2^-24 mean_r |w xhat_r| with R the rows pooled -- fp32 rounding of R terms and their sum (each term: rsqrt of a rounded
    mean square, two products and a division)."""
    B, T = 5, 6
    Tt = Ni + T
    g = torch.Generator().manual_seed(mode * 100 + Ni * 10 + H)
    x = torch.randn(B * Tt + 1, H, generator=g) * 2.0       # one more finite row behind the last batch entry
    w = 1.0 + 0.3 * torch.randn(H, generator=g)
    xd, wd = x.to(DEV), w.to(DEV)
    normed = _rms_ref64(x[:B * Tt], w, 1e-6).view(B, Tt, H)
    for lens in ([T, 1, 0, 3, T + 9], None):
        eff = [T] * B if lens is None else [min(max(n, 0), T) for n in lens]
        ld = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
        out = _sent32((B + 1) * H).view(B + 1, H)
        call(lib().fv_op_pool_norm(xd.data_ptr(), ld.data_ptr() if ld is not None else None, wd.data_ptr(), out.data_ptr(), B, Tt, Ni, H, 1e-6, mode, stream()), "fv_op_pool_norm")
        torch.cuda.synchronize()
        raw = out.cpu()
        assert bool((raw[B] == SENT32).all())
        got = raw[:B].view(torch.float32).double()
        for b in range(B):
            r0, r1 = (Ni + max(eff[b] - 1, 0), Ni + max(eff[b] - 1, 0) + 1) if mode == 0 else (0, Ni + eff[b])
            R = r1 - r0
            if R == 0:      # mean over no row: the reference's sum / clamp_min(count, 1e-6) of nothing
                assert bool((got[b] == 0).all())
                continue
            ref = normed[b, r0:r1].mean(dim=0)
            lim = 2.0 * (R + 8) * 2.0 ** -24 * normed[b, r0:r1].abs().mean(dim=0)
            err = (got[b] - ref).abs()
            assert bool((err <= lim).all()), f"mode {mode} Ni {Ni} H {H} lens {lens} b {b}: {float((err / lim).max()):.2f} x the bound"
