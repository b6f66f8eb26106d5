"""-m gpu: the bf16 attention (csrc/attention.hip launch_attention: attention32_kernel, attention_kernel<D, MASKED>) through fv_op_attention_bf16, and the tower's attention
backward (csrc/tower_bwd_kernels.hip launch_tower_attn_bwd: tattn_dq_kernel, tattn_dkv_kernel) through fv_op_tower_attention_bwd -- each on its own, per row, against float64.

  a. parity      per output tensor, batch entry and head the WORST row against the RMS row norm of the same block of the float64 reference, within 2 x the measure of the CPU
                 emulation of the kernel's arithmetic on the same inputs (tests/tower_attn_ref_util.py; the emulations' own measure is capped on the CPU by
                 tests/test_tower_attention_reference_host.py); lse2 within 2 x the emulation's absolute error + 2^-20 |lse2| (v_log_f32 / v_exp_f32)
  b. selection   one-hot softmax rows: output row i == V row pi(i) bit for bit on every route; backward dV row j == the sum of the dO rows that select j, dQ == dK == 0,
                 lse2 and delta exact -- every slot <-> key pairing and both transposing LDS reads at every key position
  c. constant V  attention32_kernel returns c_d bit for bit (numerator and row sum hold the same rounded P) with its rescale branch taken and skipped; attention_kernel
                 (rounded numerator over an un-rounded sum) stays within one bf16 ulp, and the count of elements off by one is printed
  d. footprint   sentinels around every output and behind `stats`, inputs untouched, two calls bit-identical (inside every run / the parity tests); finite values in the
                 rows >= len change no bit below len; a ragged backward result does not depend on what the neighbouring batch entries hold
  e. refusals    what the launchers refuse is refused before anything is enqueued

Measured on an MI355X: docs/kernels.md "bf16 attention and the tower's attention backward: op-level float64 parity"."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import tower_attn_ref_util as R  # noqa: E402
from gpu_util import DEV, call, lib, stream  # noqa: E402

SENT_BF16 = 0x7FA5         # a bf16 NaN pattern no kernel writes
SENT_F16 = 0x7DA5          # an fp16 NaN pattern
SENT32 = 0x7FC5A5A5        # an fp32 NaN pattern
TAIL = 8                   # extra floats behind stats


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device (no CPU fallback in the product path)")


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _padded(t2d, ld, g, dtype):
    """(rows, w) fp32 -> device (rows, ld) of dtype with the data in the first w columns and other finite values in the padding"""
    rows, w = t2d.shape
    buf = torch.randn(rows, ld, generator=g) * 3.0
    buf[:, :w] = t2d
    return buf.to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------------------- forward
def _run_fwd(c, q, k, v):
    """one fv_op_attention_bf16 call at case c's settings: every leading dimension wider than its minimum (one packed [q | k | v] buffer, or three allocations with three
    different strides), the output pre-filled with sentinels plus one extra row.  Asserts what holds for ANY inputs -- padding columns and the extra row untouched, inputs
    unchanged, every output row written -- and returns the CPU output (B, T, heads, D) fp32."""
    B, T, heads, kv, D = c.B, c.T, c.heads, c.kv, c.D
    rows, qd, kd = B * T, heads * D, kv * D
    g = torch.Generator().manual_seed(11)
    q2, k2, v2 = q.reshape(rows, qd), k.reshape(rows, kd), v.reshape(rows, kd)
    if c.separate:
        ldq, ldk, ldv = qd + R.PAD, kd + R.PAD + 8, kd + R.PAD + 24
        bufs = [_padded(q2, ldq, g, torch.bfloat16), _padded(k2, ldk, g, torch.bfloat16), _padded(v2, ldv, g, torch.bfloat16)]
        ptrs = [b.data_ptr() for b in bufs]
    else:
        ldq = ldk = ldv = qd + 2 * kd + R.PAD
        bufs = [_padded(torch.cat([q2, k2, v2], dim=1), ldq, g, torch.bfloat16)]
        ptrs = [bufs[0].data_ptr(), bufs[0].data_ptr() + 2 * qd, bufs[0].data_ptr() + 2 * (qd + kd)]
    before = [b.clone() for b in bufs]
    ldo = qd + R.PAD
    out = torch.full((rows + 1, ldo), SENT_BF16, dtype=torch.int16, device=DEV)
    l_dev = torch.tensor(c.lens, dtype=torch.int32, device=DEV) if c.lens is not None else None
    call(lib().fv_op_attention_bf16(ptrs[0], ptrs[1], ptrs[2], ldq, ldk, ldv, out.data_ptr(), ldo, B, T, heads, kv, D, int(c.causal),
                                    l_dev.data_ptr() if l_dev is not None else None, c.len_add, c.scale, stream()), f"fv_op_attention_bf16 {c.name}")
    torch.cuda.synchronize()
    raw = out.cpu()
    assert bool((raw[:rows, qd:] == SENT_BF16).all()), f"{c.name}: padding columns of out written"
    assert bool((raw[rows] == SENT_BF16).all()), f"{c.name}: the row past the end of out written"
    for b, b0 in zip(bufs, before):
        assert torch.equal(_bits16(b.cpu()), _bits16(b0.cpu())), f"{c.name}: an input was written"
    o = raw[:rows, :qd].contiguous().view(torch.bfloat16).float().view(B, T, heads, D)
    assert bool(torch.isfinite(o).all()), f"{c.name}: an output value is not finite (or was never written)"
    return o


@functools.lru_cache(maxsize=None)
def _fwd_base(name, kind):
    r = R.forward_reference(name, kind)
    return _run_fwd(r["case"], r["q"], r["k"], r["v"])


@pytest.mark.parametrize("kind", R.FWD_KINDS)
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_attention_bf16_worst_row_against_float64(name, kind):
    r = R.forward_reference(name, kind)
    c = r["case"]
    got = _fwd_base(name, kind)
    m = R.forward_measure(got, r["o64"], c)
    print(f"[{name} {kind}] {c.route}: MI355X {m:.2e} / emulation {r['emu_measure']:.2e}")
    assert r["emu_measure"] <= R.CAPS["forward"]
    assert m <= 2.0 * r["emu_measure"], f"{name} {kind}: worst row {m:.3e} > 2 x emulation {r['emu_measure']:.3e}"
    again = _run_fwd(c, r["q"], r["k"], r["v"])
    assert torch.equal(_bits16(again.bfloat16()), _bits16(got.bfloat16())), f"{name} {kind}: two identical calls differ"


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_attention_bf16_selects_exactly(name):
    """P is one-hot and the row sum exactly 1: output row i of head h is V row pi(i) bit for bit (every query its own key: permutations where nothing is masked, otherwise
    a random visible key) -- a wrong slot <-> key pairing anywhere in the V fragment order moves a row"""
    c = R.CASE_BY_NAME[name]
    q, k, v, pi = R.selection_inputs(c)
    got = _run_fwd(c, q, k, v)
    want = R.selection_expected(v, pi, c)
    bad = (got != want).any(dim=-1)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} output rows are not the selected V row; first (b, i, h): {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_attention_bf16_constant_v(name):
    """V column d constant over the keys: attention32_kernel must return c_d bit for bit in every row (plain, plateau, every rescale skipped after the first tile, every
    rescale taken); attention_kernel within one bf16 ulp of c_d -- the elements off by one are the cost of dividing a rounded numerator by an un-rounded sum"""
    c = R.CASE_BY_NAME[name]
    for kind in R.FWD_KINDS:
        for variant in R.constant_v_variants(c, kind):
            q, k, v, cd = R.constant_v_inputs(c, kind, variant)
            dev, off, n = R.constant_v_deviation(_run_fwd(c, q, k, v), cd, c)
            print(f"[{name} {kind} {variant}] {c.route}: {off} of {n} elements differ from c_d, worst {float(dev.max()):.2f} ulp")
            if c.route == "attention32_kernel":
                assert off == 0, f"{name} {kind} {variant}: {off} of {n} elements differ from c_d"
            else:
                ok = R.valid_rows(c)[:, :, None, None].expand_as(dev)
                assert float(dev[ok].max()) <= 1.0, f"{name} {kind} {variant}: {float(dev[ok].max())} ulp from c_d"


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.lens is not None and min(c.key_lens()) < c.T])
def test_attention_bf16_rows_past_len_change_nothing_below_it(name):
    """other FINITE values (|x| <= 1e4) in the rows >= klen of q, k and v leave every output row < klen bit-identical.  (Not NaN / Inf: masked keys enter the P.V product on
    the matrix core with P = 0, and 0 x NaN is NaN -- padding must be finite; docs/kernels.md.)"""
    r = R.forward_reference(name, "gauss")
    c = r["case"]
    got = _fwd_base(name, "gauss")
    g = torch.Generator().manual_seed(5)
    q2, k2, v2 = r["q"].clone(), r["k"].clone(), r["v"].clone()
    for b, n in enumerate(c.key_lens()):
        for t, amp in ((q2, 50.0), (k2, 50.0), (v2, 1e4)):
            t[b, n:] = R.bf((torch.rand(t[b, n:].shape, generator=g) * 2.0 - 1.0) * amp)
    other = _run_fwd(c, q2, k2, v2)
    ok = R.valid_rows(c)
    assert torch.equal(_bits16(other[ok].bfloat16()), _bits16(got[ok].bfloat16())), f"{name}: rows < klen depend on the rows >= klen"


# --------------------------------------------------------------------------------------------------------------------------------------------- backward
def _run_bwd(B, T, heads, qkv, dO):
    """one fv_op_tower_attention_bwd call, ld / lddo / ldd PAD wider than their minimum, dqkv pre-filled with sentinels plus one extra row, stats with a sentinel tail.
    Asserts sentinels, untouched inputs and that everything else was written; returns CPU dq, dk, dv (B, T, heads, 32) fp32, lse2, delta (B, heads, T) and the raw bits."""
    C, rows = 32 * heads, B * T
    ld, lddo, ldd = 3 * C + R.PAD, C + R.PAD, 3 * C + R.PAD
    g = torch.Generator().manual_seed(13)
    x_dev, g_dev = _padded(qkv.reshape(rows, 3 * C), ld, g, torch.bfloat16), _padded(dO.reshape(rows, C), lddo, g, torch.float16)
    x0, g0 = x_dev.clone(), g_dev.clone()
    dqkv = torch.full((rows + 1, ldd), SENT_F16, dtype=torch.int16, device=DEV)
    nstat = 2 * B * heads * T
    stats = torch.full((nstat + TAIL,), SENT32, dtype=torch.int32, device=DEV)
    call(lib().fv_op_tower_attention_bwd(x_dev.data_ptr(), ld, g_dev.data_ptr(), lddo, dqkv.data_ptr(), ldd, stats.data_ptr(), B, T, heads, R.f32_scale(32), stream()),
         f"fv_op_tower_attention_bwd B={B} T={T} heads={heads}")
    torch.cuda.synchronize()
    draw, sraw = dqkv.cpu(), stats.cpu()
    assert bool((draw[:rows, 3 * C:] == SENT_F16).all()), "padding columns of dqkv written"
    assert bool((draw[rows] == SENT_F16).all()), "the row past the end of dqkv written"
    assert bool((sraw[nstat:] == SENT32).all()), "stats written past 2 B heads T"
    assert torch.equal(_bits16(x_dev.cpu()), _bits16(x0.cpu())) and torch.equal(_bits16(g_dev.cpu()), _bits16(g0.cpu())), "an input was written"
    body = draw[:rows, :3 * C].contiguous()
    gr = body.view(torch.float16).float().view(B, T, 3, heads, 32)
    st = sraw[:nstat].contiguous().view(torch.float32).view(2, B, heads, T)
    assert bool(torch.isfinite(gr).all()) and bool(torch.isfinite(st).all()), "an output value is not finite (or was never written)"
    return {"dq": gr[:, :, 0], "dk": gr[:, :, 1], "dv": gr[:, :, 2], "lse2": st[0], "delta": st[1], "raw": (body, sraw[:nstat].contiguous())}


@functools.lru_cache(maxsize=None)
def _bwd_base(name, kind):
    r = R.backward_reference(name, kind)
    c = r["case"]
    return _run_bwd(c.B, c.T, c.heads, r["qkv"], r["dO"])


@pytest.mark.parametrize("kind", R.BWD_KINDS)
@pytest.mark.parametrize("name", [c.name for c in R.BWD_CASES])
def test_tower_attention_bwd_worst_rows_against_float64(name, kind):
    r = R.backward_reference(name, kind)
    c = r["case"]
    got = _bwd_base(name, kind)
    m, emu = R.backward_measures(got["dq"], got["dk"], got["dv"], got["lse2"], got["delta"], r), r["emu_measures"]
    print(f"[{name} {kind}] " + "  ".join(f"{k} {m[k]:.2e} / {emu[k]:.2e}" for k in m) + "   (MI355X / emulation)")
    for k in ("dq", "dk", "dv"):
        assert emu[k] <= R.CAPS[(kind, k)]
        assert m[k] <= 2.0 * emu[k], f"{name} {kind}: worst {k} row {m[k]:.3e} > 2 x emulation {emu[k]:.3e}"
    assert m["delta"] <= 2.0 * emu["delta"], f"{name} {kind}: delta {m['delta']:.3e} > 2 x emulation {emu['delta']:.3e}"
    slack = 2.0 ** -20 * float(r["lse2_64"].abs().max())
    assert m["lse2"] <= 2.0 * emu["lse2"] + slack, f"{name} {kind}: lse2 {m['lse2']:.3e} > 2 x emulation {emu['lse2']:.3e} + {slack:.1e}"
    again = _run_bwd(c.B, c.T, c.heads, r["qkv"], r["dO"])
    assert torch.equal(again["raw"][0], got["raw"][0]) and torch.equal(again["raw"][1], got["raw"][1]), f"{name} {kind}: two identical calls differ"


@pytest.mark.parametrize("many", [False, True], ids=["permutation", "many_to_one"])
@pytest.mark.parametrize("name", [c.name for c in R.BWD_CASES])
def test_tower_attention_bwd_selects_exactly(name, many):
    """one-hot P in fp16: dV row j is the sum of the dO rows whose query selects key j (a permutation: exactly one row), bit for bit; lse2 is the selected score and delta the
    selected dP, exactly; and since delta comes from the same single exponential, dP - delta is an exact 0: dQ and dK are exactly zero"""
    c = R.BWD_BY_NAME[name]
    qkv, dO, pi = R.bwd_selection_inputs(c, many)
    got = _run_bwd(c.B, c.T, c.heads, qkv, dO)
    dv, lse2, delta = R.bwd_selection_expected(qkv, dO, pi, c)
    bad = (got["dv"] != dv).any(dim=-1)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} dV rows are not the sum of the selecting dO rows; first (b, j, h): {bad.nonzero()[0].tolist()}"
    assert torch.equal(got["lse2"], lse2), f"{name}: lse2 is not the selected score ({float((got['lse2'] - lse2).abs().max()):.3e})"
    assert torch.equal(got["delta"], delta), f"{name}: delta is not the selected dP ({float((got['delta'] - delta).abs().max()):.3e})"
    assert bool((got["dq"] == 0).all()), f"{name}: dQ is not exactly zero (max {float(got['dq'].abs().max()):.3e})"
    assert bool((got["dk"] == 0).all()), f"{name}: dK is not exactly zero (max {float(got['dk'].abs().max()):.3e})"


@pytest.mark.parametrize("name", [c.name for c in R.BWD_CASES if c.T % 64])
def test_tower_attention_bwd_neighbouring_batch_entries_do_not_leak(name):
    """ragged T: keys / queries past T are read from a clamped row and masked.  The result of the case's rows must not change by a bit when they are the first entries of a
    B + 1 call whose last entry holds other data, nor when that other entry comes first"""
    r = R.backward_reference(name, "gauss")
    c = r["case"]
    got = _bwd_base(name, "gauss")
    g = torch.Generator().manual_seed(21)
    oq = R.bf(torch.randn(1, c.T, 3 * c.C, generator=g) * 2.0 + 0.5)
    og = R.h16(torch.randn(1, c.T, c.C, generator=g) * 3.0 - 0.5)
    for first in (True, False):
        parts = ([r["qkv"], oq], [r["dO"], og]) if first else ([oq, r["qkv"]], [og, r["dO"]])
        big = _run_bwd(c.B + 1, c.T, c.heads, torch.cat(parts[0]), torch.cat(parts[1]))
        sl = slice(0, c.B) if first else slice(1, c.B + 1)
        for k in ("dq", "dk", "dv", "lse2", "delta"):
            assert torch.equal(big[k][sl].contiguous().view(torch.int32), got[k].contiguous().view(torch.int32)), \
                f"{name}: {k} depends on a neighbouring batch entry (the case's rows {'first' if first else 'last'})"


# --------------------------------------------------------------------------------------------------------------------------------------------- refusals
def test_wrappers_refuse_what_the_launchers_refuse():
    """each refusal returns an error with the launcher's message, before anything is enqueued: every buffer still holds its sentinel afterwards"""
    L = lib()
    B, T, heads, kv, D = 1, 64, 4, 2, 64
    qd, kd = heads * D, kv * D
    w = qd + 2 * kd
    buf = torch.zeros(B * T, w + 16, dtype=torch.bfloat16, device=DEV)
    out = torch.full((B * T, qd + 16), SENT_BF16, dtype=torch.int16, device=DEV)
    p0 = buf.data_ptr()

    def refused_fwd(word, *, q=p0, k=p0 + 2 * qd, v=p0 + 2 * (qd + kd), ldq=w, ldk=w, ldv=w, o=out.data_ptr(), ldo=qd, heads=heads, kv=kv, D=D):
        rc = L.fv_op_attention_bf16(q, k, v, ldq, ldk, ldv, o, ldo, B, T, heads, kv, D, 1, None, 0, 0.125, stream())
        msg = L.fv_last_error(None).decode()
        assert rc != 0, f"accepted: {word}"
        assert "attention" in msg and word in msg, (word, msg)

    for name in ("q", "k", "v", "o"):
        refused_fwd("null", **{name: None})
    refused_fwd("heads=5", heads=5, kv=2)
    refused_fwd("multiples of 8", ldq=w + 4)
    refused_fwd("multiples of 8", ldv=w + 2)
    refused_fwd("multiples of 8", ldo=qd + 2)
    refused_fwd("smaller than", ldq=qd - 8)
    refused_fwd("smaller than", ldk=kd - 8)
    refused_fwd("smaller than", ldo=qd - 4)
    refused_fwd("misaligned", k=p0 + 2 * qd + 2)
    refused_fwd("misaligned", o=out.data_ptr() + 2)
    refused_fwd("head_dim 48", D=48, heads=2, kv=2)

    C = 32 * heads
    x = torch.zeros(B * T, 3 * C + 16, dtype=torch.bfloat16, device=DEV)
    gO = torch.zeros(B * T, C + 16, dtype=torch.float16, device=DEV)
    dqkv = torch.full((B * T, 3 * C + 16), SENT_F16, dtype=torch.int16, device=DEV)
    stats = torch.full((2 * B * heads * T,), SENT32, dtype=torch.int32, device=DEV)

    def refused_bwd(word, *, x_p=x.data_ptr(), ld=3 * C, g_p=gO.data_ptr(), lddo=C, d_p=dqkv.data_ptr(), ldd=3 * C, s_p=stats.data_ptr(), heads=heads):
        rc = L.fv_op_tower_attention_bwd(x_p, ld, g_p, lddo, d_p, ldd, s_p, B, T, heads, R.f32_scale(32), stream())
        msg = L.fv_last_error(None).decode()
        assert rc != 0, f"accepted: {word}"
        assert "tower_attn_bwd" in msg and word in msg, (word, msg)

    for name in ("x_p", "g_p", "d_p", "s_p"):
        refused_bwd("null", **{name: None})
    refused_bwd("strides", ld=3 * C - 8)
    refused_bwd("strides", lddo=C - 8)
    refused_bwd("strides", ldd=3 * C - 8)
    refused_bwd("strides", ld=3 * C + 4)
    refused_bwd("strides", lddo=C + 4)
    refused_bwd("strides", ldd=3 * C + 2)
    refused_bwd("strides", heads=0)
    refused_bwd("misaligned", x_p=x.data_ptr() + 2)
    refused_bwd("misaligned", d_p=dqkv.data_ptr() + 8)
    torch.cuda.synchronize()
    for name, b, sent in (("out", out, SENT_BF16), ("dqkv", dqkv, SENT_F16), ("stats", stats, SENT32)):
        assert bool((b == sent).all()), f"a refused call wrote {name}"
    assert bool((buf == 0).all()) and bool((x == 0).all()) and bool((gO == 0).all())
