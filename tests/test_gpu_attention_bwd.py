"""-m gpu: the backward of the decoder's fp32 attention, every route launch_attention_bwd (csrc/train_kernels.hip) can take, each on its own against float64
autograd of the same operator, through the test-only entry point fv_op_attention_bwd_routes (include/fastvla_hip_testops.h):

  split route   attn_prep_kv_kernel, attn_fwd_split_kernel (the lse), attn_bwd_dq_split_kernel<D, grouped | per head>, attn_bwd_dkv_split_kernel<D, PART | looped>
  fp32 route    attention_f32_mfma_kernel (the lse), attn_bwd_dq_kernel<D>, attn_bwd_dkv_kernel<D, PART | looped>       (no scratch buffer)
  both          attn_dkv_reduce_kernel when `part` is given and the GQA group has more than one q head -- the training step's own configuration, with len_add = Ni

at the smallest shapes that cross each tile, block and record edge (tests/attn_bwd_ref_util.py SHAPES / CASES, checked in tests/test_attention_bwd_reference_host.py).

Measure: per gradient (dq, dk, dv), batch entry and head the WORST ROW < klen against the RMS row norm of the same block of the float64 reference
(attn_bwd_ref_util.block_measure; a gradient row's own norm can be exactly zero), delta in absolute error against RMS ||dO_i|| ||o_i||.  Bound: 2 x the measure of the
matching CPU emulation of the route's arithmetic on the same inputs (the factor covers __expf and the order inside a step; the fp32 route's emulation accumulates
its products one at a time in the kernels' order, because dV's error there IS the length of that chain; the emulations' own error is capped on the CPU).
Everything else is an exact-bit property: zeros past klen, sentinels around every output, untouched inputs, repeatability, masking, and the k | v columns as the
in-order fp32 sum of the per-q-head shares.

Measured on an MI355X (worst case of each class, GPU / emulation): docs/kernels.md "Attention backward: op-level float64 parity"."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_bwd_ref_util as R  # noqa: E402
from gpu_util import DEV, call, lib, stream  # noqa: E402

SENT16 = 0x7FA5            # a bf16 NaN pattern no kernel writes
SENT32 = 0x7FC5A5A5        # an fp32 NaN pattern
TAIL = 8                   # extra elements behind stat and part


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device (no CPU fallback in the product path)")


def _padded(t2d, ld, g):
    """(rows, w) fp32 -> device (rows, ld) with the data in the first w columns and other finite values in the padding"""
    rows, w = t2d.shape
    buf = torch.randn(rows, ld, generator=g) * 3.0
    buf[:, :w] = t2d
    return buf.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(c, qkv, dO):
    """one fv_op_attention_bwd_routes call at case c's settings, every leading dimension PAD wider than its minimum, every output pre-filled with sentinels and one
    extra row / tail.  Asserts what must hold for ANY inputs (sentinels, inputs untouched, `part` ignored when it must be) and returns CPU tensors: dq (B, T, heads, D),
    dk, dv (B, T, kv, D) fp32, lse, delta (B, heads, T), shares (group, B T, 2 kd) or None, raw = the int32 bits of (dqkv body, stat body)."""
    s = c.shape
    B, T, heads, kv, D = s.B, s.T, s.heads, s.kv, s.D
    qd, kd, grp, rows = heads * D, kv * D, heads // kv, B * T
    w = qd + 2 * kd
    ld, lddo, ldo = w + R.PAD, qd + R.PAD, 2 * qd + R.PAD
    g = torch.Generator().manual_seed(11)
    q_dev, g_dev = _padded(qkv.reshape(rows, w), ld, g), _padded(dO.reshape(rows, qd), lddo, g)
    q_before, g_before = q_dev.clone(), g_dev.clone()
    l_dev = torch.tensor(s.lens, dtype=torch.int32, device=DEV) if s.lens is not None else None
    dqkv = torch.full((rows + 1, ld), SENT32, dtype=torch.int32, device=DEV)
    out = torch.full((rows + 1, ldo), SENT16, dtype=torch.int16, device=DEV)
    nstat, npart = 2 * B * heads * T, grp * rows * 2 * kd
    stat = torch.full((nstat + TAIL,), SENT32, dtype=torch.int32, device=DEV)
    part = torch.full((npart + TAIL,), SENT32, dtype=torch.int32, device=DEV) if c.parts else None
    call(lib().fv_op_attention_bwd_routes(q_dev.data_ptr(), ld, g_dev.data_ptr(), lddo, dqkv.data_ptr(), out.data_ptr(), ldo, stat.data_ptr(),
                                          part.data_ptr() if c.parts else None, B, T, heads, kv, D, l_dev.data_ptr() if l_dev is not None else None, s.len_add,
                                          R.A.THETA, int(c.use_split), stream()), f"fv_op_attention_bwd_routes {c.name}")
    torch.cuda.synchronize()
    draw, sraw, oraw = dqkv.cpu(), stat.cpu(), out.cpu()
    assert bool((draw[:rows, w:] == SENT32).all()), f"{c.name}: padding columns of dqkv written"
    assert bool((draw[rows] == SENT32).all()), f"{c.name}: the row past the end of dqkv written"
    assert bool((sraw[nstat:] == SENT32).all()), f"{c.name}: stat written past 2 B heads T"
    assert bool((oraw[:rows, 2 * qd:] == SENT16).all()) and bool((oraw[rows] == SENT16).all()), f"{c.name}: the forward output's padding / extra row written"
    assert torch.equal(_bits(q_dev.cpu()), _bits(q_before.cpu())), f"{c.name}: qkv was written"
    assert torch.equal(_bits(g_dev.cpu()), _bits(g_before.cpu())), f"{c.name}: dO was written"
    body = draw[:rows, :w].contiguous()
    dq, dk, dv = R.split_grads(body.view(torch.float32).view(B, T, w), s)
    st = sraw[:nstat].contiguous().view(torch.float32).view(2, B, heads, T)
    shares = None
    if c.parts:
        praw = part.cpu()
        assert bool((praw[npart:] == SENT32).all()), f"{c.name}: part written past group x B T x 2 kd"
        if c.part_kernels:
            shares = praw[:npart].contiguous().view(torch.float32).view(grp, rows, 2 * kd)
        else:
            assert bool((praw == SENT32).all()), f"{c.name}: part written although the group has one q head"
    return {"dq": dq, "dk": dk, "dv": dv, "lse": st[0], "delta": st[1], "shares": shares, "raw": (body, sraw[:nstat].contiguous())}


@functools.lru_cache(maxsize=None)
def _base(name):
    c = R.CASE_BY_NAME[name]
    r = R.reference(*c.ref_key)
    return _run(c, r["qkv"], r["dO"])


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_attention_bwd_worst_rows_against_float64(name):
    """Every route, dq form and dK / dV form at its case's shape: the worst row of dq, dk, dv and delta against float64 within twice the emulation's own (which is
    under its cap); every value written and finite; exact zeros on the rows >= klen (dK / dV: masked keys; dQ and delta: dO is zero there); a second call
    bit-identical; with `part`, the k | v columns are the fp32 sum of the per-q-head shares in the order 0, 1, ... bit for bit."""
    c = R.CASE_BY_NAME[name]
    s = c.shape
    r = R.reference(*c.ref_key)
    got = _base(name)
    for k in ("dq", "dk", "dv", "lse", "delta"):
        assert bool(torch.isfinite(got[k]).all()), f"{name}: {k} holds a value that is not finite (or was never written)"
    m, emu = R.measures(got["dq"], got["dk"], got["dv"], got["delta"], r), r["emu_measures"]
    print(f"[{name}] " + "  ".join(f"{k} {m[k]:.2e} (emulation {emu[k]:.2e})" for k in m) + f"  cap {c.cap:.1e}")
    for k in m:
        assert emu[k] <= c.cap, f"{name}: the emulation's {k} {emu[k]:.3e} is over its cap {c.cap:.1e}"
        assert m[k] <= 2.0 * emu[k], f"{name}: worst {k} row {m[k]:.3e} > 2 x emulation {emu[k]:.3e}"
    for b, n in enumerate(c.key_lens()):
        for k in ("dq", "dk", "dv"):
            assert bool((got[k][b, n:] == 0).all()), f"{name}: {k} of batch entry {b} is not exactly zero on the rows >= {n}"
        assert bool((got["delta"][b, :, n:] == 0).all()), f"{name}: delta of batch entry {b} is not exactly zero on the rows >= {n}"
    again = _run(c, r["qkv"], r["dO"])
    assert torch.equal(again["raw"][0], got["raw"][0]) and torch.equal(again["raw"][1], got["raw"][1]), f"{name}: two identical calls differ"
    if c.part_kernels:
        qd, kd = s.heads * s.D, s.kv * s.D
        sh = got["shares"]
        assert bool(torch.isfinite(sh).all()), f"{name}: a share was not written"
        acc = sh[0].clone()
        for g in range(1, c.group):
            acc = acc + sh[g]
        assert torch.equal(_bits(acc), got["raw"][0][:, qd:qd + 2 * kd].contiguous()), f"{name}: dk | dv is not the in-order fp32 sum of the shares"


@pytest.mark.parametrize("name", [c.name for c in R.CASES if min(c.key_lens()) < c.shape.T])
def test_attention_bwd_rows_past_the_prompt_change_nothing_below_it(name):
    """The kernels mask qi < len and kj < len, so (a) finite garbage in the dO rows >= klen leaves all of dK and dV, and dQ on the rows < klen, bit-identical, and
    (b) other finite values in the qkv rows >= klen leave every gradient row < klen and delta there bit-identical (masked terms are exact zeros)."""
    c = R.CASE_BY_NAME[name]
    s = c.shape
    r = R.reference(*c.ref_key)
    got = _base(name)
    klens = c.key_lens()
    below = (torch.arange(s.T)[None, :] < torch.tensor(klens)[:, None])           # (B, T)
    gg = torch.Generator().manual_seed(5)
    dO2, q2 = r["dO"].clone(), r["qkv"].clone()
    for b, n in enumerate(klens):
        dO2[b, n:] = torch.randn(dO2[b, n:].shape, generator=gg) * 5.0 + 1.0
        q2[b, n:] = torch.randn(q2[b, n:].shape, generator=gg) * 5.0 + 1.0
    a = _run(c, r["qkv"], dO2)
    assert torch.equal(_bits(a["dk"]), _bits(got["dk"])) and torch.equal(_bits(a["dv"]), _bits(got["dv"])), f"{name}: dK / dV depend on the dO rows >= klen"
    assert torch.equal(_bits(a["dq"][below]), _bits(got["dq"][below])), f"{name}: dQ rows < klen depend on the dO rows >= klen"
    b_ = _run(c, q2, r["dO"])
    for k in ("dq", "dk", "dv"):
        assert torch.equal(_bits(b_[k][below]), _bits(got[k][below])), f"{name}: {k} rows < klen depend on the qkv rows >= klen"
    d1, d0 = b_["delta"].transpose(1, 2)[below], got["delta"].transpose(1, 2)[below]
    assert torch.equal(_bits(d1), _bits(d0)), f"{name}: delta rows < klen depend on the qkv rows >= klen"


def test_attention_bwd_routes_wrapper_rejects_what_it_cannot_run():
    """each refusal returns an error with its own message, before anything is enqueued: every buffer still holds its sentinel afterwards"""
    L = lib()
    B, T, heads, kv, D = 1, 8, 4, 2, 64
    qd, w = heads * D, (heads + 2 * kv) * D
    qkv = torch.zeros(B * T, w + 16, device=DEV)
    dO = torch.zeros(B * T, qd + 16, device=DEV)
    dqkv = torch.full((B * T, w + 16), SENT32, dtype=torch.int32, device=DEV)
    out = torch.full((B * T, 2 * qd + 16), SENT16, dtype=torch.int16, device=DEV)
    stat = torch.full((2 * B * heads * T,), SENT32, dtype=torch.int32, device=DEV)
    part = torch.full((2 * B * T * 2 * kv * D,), SENT32, dtype=torch.int32, device=DEV)

    def refused(word, *, qkv_p=qkv.data_ptr(), ld=w, dO_p=dO.data_ptr(), lddo=qd, dq_p=dqkv.data_ptr(), out_p=out.data_ptr(), ldo=2 * qd, stat_p=stat.data_ptr(),
                heads=heads, kv=kv, D=D, split=1):
        rc = L.fv_op_attention_bwd_routes(qkv_p, ld, dO_p, lddo, dq_p, out_p, ldo, stat_p, part.data_ptr(), B, T, heads, kv, D, None, 0, 1e6, split, stream())
        msg = L.fv_last_error(None).decode()
        assert rc != 0, f"accepted: {word}"
        assert "attention_bwd" in msg and word in msg, (word, msg)

    for split in (0, 1):
        refused("head_dim", D=32, split=split)
        refused("ld =", ld=w + 2, split=split)
        refused("ld =", ld=w - 4, split=split)
        refused("lddo", lddo=qd + 2, split=split)
        refused("lddo", lddo=qd - 4, split=split)
        refused("ldo", ldo=2 * qd + 4, split=split)
        refused("ldo", ldo=2 * qd - 8, split=split)
        refused("multiple of kv_heads", heads=5, kv=2, split=split)
        for k in ("qkv_p", "dO_p", "dq_p", "out_p", "stat_p"):
            refused("null", split=split, **{k: None})
    torch.cuda.synchronize()
    for name, buf, sent in (("dqkv", dqkv, SENT32), ("out", out, SENT16), ("stat", stat, SENT32), ("part", part, SENT32)):
        assert bool((buf == sent).all()), f"a refused call wrote {name}"
    assert bool((qkv == 0).all()) and bool((dO == 0).all())
