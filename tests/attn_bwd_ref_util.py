"""CPU references for the BACKWARD of the decoder's fp32 attention (csrc/train_kernels.hip launch_attention_bwd: the fp32-MFMA kernels attn_bwd_dq_kernel /
attn_bwd_dkv_kernel, the split-bf16 kernels of csrc/attention_split.hip, attn_dkv_reduce_kernel), shared by tests/test_attention_bwd_reference_host.py (no GPU)
and tests/test_gpu_attention_bwd.py.  TEST INFRASTRUCTURE ONLY; the forward's references (tests/attn_ref_util.py) are imported, not repeated.

The operator: the gradient of sum(dO o o) with o = the causal GQA attention of attn_ref_util.attention (rotate-half RoPE of the fp32 table inside, key j visible
to query i iff j <= i and j < klen = clamp(lens[b] + len_add, 1, T)), with respect to the UN-rotated packed rows [q | k | v]; dO is zero on the rows >= klen (the
training step's loss never reads them).  Three forms:

  reference      torch.autograd through attention(..., mode="f64"), and delta = sum_d dO o in float64
  form "exact"   the fp32-MFMA route, from the header comment of the kernels (train_kernels.hip "attention backward"): everything in torch fp32, lse from the fp32
                 forward emulation, P = exp(S scale - lse), dP = dO V^T, delta = sum dO o round_out(o) -- the kernels read the forward's 16-bit output hi + lo --,
                 dS = P o (dP - delta) scale, dQ = dS K, dK = dS^T Q, dV = P^T dO with the queries >= klen left out of dK / dV, the gradients rotated back.
                 The three gradient products are ACCUMULATED AS THE KERNELS DO (_chain): one fp32 accumulator per output element, one fused multiply-add per
                 product, over the keys (dQ) or over the group's q heads and their queries (dK / dV) in the kernels' order -- a chain of up to heads/kv x T
                 roundings, whose error (~sqrt(n) 2^-24) is what dV's consists of; with `part` one chain per q head and the shares added in order
  form "split"   the split-bf16 route (attention_split.hip header): the same with every product formed as hi.hi + lo.hi + hi.lo on split_bf16 operands (_mm3), P and
                 dS split again before the second products (split8(p), split8(ds)), the forward in mode "split"

Measure (block_measure): per gradient (dq, dk, dv), batch entry and head (q head, or kv head for dk / dv), over the rows < klen:
max_row ||got - ref|| / RMS_rows ||ref||, norms over the head's D values; the maximum over batch entries and heads.  The row's own norm is NOT the scale: dQ of
query 0 is exactly zero (one visible key: dS = 0) and peaked rows have tiny gradients.  A block whose reference vanishes identically -- a key length of 1: dQ and dK
are zero, while the kernels' dP - delta is the 16-bit rounding of o, not zero -- has no RMS; it is measured against the size its rows would have with |dP - delta| at
its bound, scale x RMS_i(||dO_i|| ||o_i||) x RMS ||k_j|| (for dK: ||q_i||).  delta: max |got - ref| / RMS_i(||dO_i|| ||o_i||) per (batch, q head).

CASES are what the GPU tests run; the host test holds the emulations' own measure under CAPS at every one of them, so the GPU bound (2 x the emulation under the
same measure on the same inputs: __expf and summation order, the forward tests' factor) cannot hide a wrong kernel behind a loose emulation."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

import attn_ref_util as A

PAD = A.PAD
# the emulations' own worst row (block_measure, the worst of dq / dk / dv, and delta) must stay under these: conditions, not tolerances.  About twice what the
# emulations measure at D = 64 and 128 (INPUT_SCALE inputs: exact <= 2.9e-5, split <= 5.4e-5; peaked: 3.0e-5 / 1.1e-4).
CAPS = {("plain", "exact"): 4e-5, ("plain", "split"): 1e-4, ("peaked", "exact"): 6e-5, ("peaked", "split"): 3e-4}
PEAK = 3.0            # the peaked case multiplies the q and k columns by this


@dataclass(frozen=True)
class Shape:
    name: str
    B: int
    T: int
    heads: int
    kv: int
    D: int
    lens: Optional[Tuple[int, ...]] = None
    len_add: int = 0
    peaked: bool = False


@dataclass(frozen=True)
class Case:
    shape: Shape
    use_split: bool
    parts: bool

    @property
    def name(self) -> str:
        return f"{self.shape.name}-{'split' if self.use_split else 'fp32'}-{'parts' if self.parts else 'looped'}"

    @property
    def form(self) -> str:
        return "split" if self.use_split else "exact"

    @property
    def cap(self) -> float:
        return CAPS[("peaked" if self.shape.peaked else "plain", self.form)]

    @property
    def group(self) -> int:
        return self.shape.heads // self.shape.kv

    @property
    def grouped_dq(self) -> bool:
        """the split route's dq form: one block per GQA group, a wave per q head (launch_attention_split_bwd: 2 <= group <= 8), else one block per q head"""
        return self.use_split and 2 <= self.group <= 8

    @property
    def part_kernels(self) -> bool:
        """launch_attention_bwd: the PART instances and the reduce kernel run iff part is given and the group has more than one q head"""
        return self.parts and self.group > 1

    @property
    def ref_key(self):
        """reference(*ref_key): only the exact emulation tells the PART form of dK / dV from the looped one (the order of the fp32 accumulation)"""
        return (self.shape.name, self.form, self.part_kernels and not self.use_split)

    def key_lens(self):
        return key_lens(self.shape)


def key_lens(s: Shape):
    if s.lens is None:
        return [s.T] * s.B
    return [max(1, min(int(l) + s.len_add, s.T)) for l in s.lens]


SHAPES = [
    # lengths and masking
    Shape("ragged_T150", 2, 150, 4, 2, 64, lens=(150, 97)),                   # a ragged last block on both routes, group 2
    Shape("one_past_T129", 1, 129, 4, 2, 64),                                  # ONE key / query in the last block (128-row and 64-row) and in the last K / V record
    Shape("block_edge", 2, 150, 4, 2, 64, lens=(128, 64)),                     # lengths on a block and a record edge: whole key blocks skipped, still written as zeros
    Shape("len_one", 3, 100, 4, 2, 64, lens=(100, 83, 1)),                     # a prompt of one token: dQ and dK vanish identically there
    Shape("len_add_40", 2, 60, 4, 2, 64, lens=(5, 20), len_add=40),            # 45 / 60 keys
    Shape("len_add_50_clamps", 2, 60, 4, 2, 64, lens=(5, 20), len_add=50),     # 55 / 70 -> clamped to T
    Shape("engine_Ni64", 2, 96, 4, 2, 64, lens=(32, 9), len_add=64),           # the training step's call: lens = text lengths, len_add = Ni image tokens
    # small shapes
    Shape("single_token", 2, 1, 4, 2, 64),
    Shape("one_ragged_tile", 1, 17, 4, 2, 64),
    # head grouping
    Shape("group7_T65", 1, 65, 14, 2, 64),                                     # 7 waves per grouped block, one query in the third 32-query block; 7 shares
    Shape("no_grouping_T200", 2, 200, 2, 2, 64, lens=(200, 183)),              # group 1: part is given and must be ignored
    Shape("group9_T130", 1, 130, 9, 1, 64),                                    # a group wider than a grouped block holds: the per-head dq kernel, nine shares
    # head_dim 128 (split: NT = 1, 64-row blocks, 16-query grouped blocks; fp32: chunks of 32)
    Shape("d128_T130", 2, 130, 4, 2, 128, lens=(130, 77)),
    Shape("d128_no_grouping_T70", 1, 70, 2, 2, 128),                           # the per-head dq kernel at head_dim 128, six queries in the second block
    # peaked softmax
    Shape("peaked_T150", 2, 150, 4, 2, 64, lens=(150, 97), peaked=True),
]
SHAPE_BY_NAME = {s.name: s for s in SHAPES}
# every shape on both routes; every group > 1 with and without `part`; group 1 with `part` given (ignored)
CASES = [Case(s, r == "split", p) for s in SHAPES for r in ("split", "fp32") for p in ((False, True) if s.heads > s.kv else (True,))]
CASE_BY_NAME = {c.name: c for c in CASES}


def make_inputs(s: Shape):
    """-> qkv (B, T, (heads + 2 kv) D) fp32 un-rotated, dO (B, T, heads D) fp32 with zero rows >= klen, table (T, D/2, 2) fp32"""
    c = A.Case(s.name, s.B, s.T, s.heads, s.kv, s.D, lens=s.lens, len_add=s.len_add)
    qkv, _, table, _ = A.make_inputs(c, seed_extra=17)
    if s.peaked:
        qkv = qkv.clone()
        qkv[..., :(s.heads + s.kv) * s.D] *= PEAK
    g = torch.Generator().manual_seed(4242 + 1000 * s.B + s.T + 7 * s.heads + s.D)
    dO = torch.randn(s.B, s.T, s.heads * s.D, generator=g)
    for b, n in enumerate(key_lens(s)):
        dO[b, n:] = 0.0
    return qkv, dO, table


def split_grads(g, s: Shape):
    """(B, T, (heads + 2 kv) D) -> dq (B, T, heads, D), dk (B, T, kv, D), dv (B, T, kv, D)"""
    qd, kd = s.heads * s.D, s.kv * s.D
    return (g[..., :qd].reshape(s.B, s.T, s.heads, s.D), g[..., qd:qd + kd].reshape(s.B, s.T, s.kv, s.D),
            g[..., qd + kd:qd + 2 * kd].reshape(s.B, s.T, s.kv, s.D))


def reference_f64(qkv, dO, table, s: Shape):
    """float64 autograd -> dq, dk, dv (float64), delta (B, heads, T), o (B, T, heads, D)"""
    x = qkv.double().clone().requires_grad_(True)
    o, _ = A.attention(x, s.heads, s.kv, s.D, table, s.lens, s.len_add, None, "f64")
    w = dO.double().view(s.B, s.T, s.heads, s.D)
    (w * o).sum().backward()
    delta = (w * o.detach()).sum(-1).transpose(1, 2).contiguous()
    return (*split_grads(x.grad, s), delta, o.detach())


def autograd_f32(qkv, dO, table, s: Shape):
    """plain fp32 autograd of the fp32 form of the operator: what the exact emulation must agree with up to rounding (a wrong formula there shows here)"""
    x = qkv.clone().requires_grad_(True)
    o, _ = A.attention(x, s.heads, s.kv, s.D, table, s.lens, s.len_add, None, "f32")
    (dO.view(s.B, s.T, s.heads, s.D) * o).sum().backward()
    return split_grads(x.grad, s)


def _unrotate(g, table):
    """gradient w.r.t. the rotated rows (B, T, h, D) -> w.r.t. the un-rotated ones: (q1, q2) = (a c - b s, b c + a s) => da = g1 c + g2 s, db = g2 c - g1 s (fp32)"""
    h = g.shape[-1] // 2
    cs = table[:g.shape[1]]
    co, si = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
    g1, g2 = g[..., :h], g[..., h:]
    return torch.cat([g1 * co + g2 * si, g2 * co - g1 * si], dim=-1)


def _mfma_order(n: int):
    """the order in which the fp32 kernels feed rows (keys or queries) 0 .. n - 1 to an accumulator: tiles of 16 ascending; within a tile four
    v_mfma_f32_16x16x4_f32 (r = 0 .. 3), each contracting the rows 4 fg + r, fg = 0 .. 3 (train_kernels.hip attn_bwd_dq_kernel `dq[dt] = mfma(kc[r * LDR ..], ds[r], ..)`,
    attn_bwd_dkv_kernel `dv[dt] = mfma(dcol[r * LDR ..], p[r], ..)` / `dk[dt] = mfma(qcol[r * LDR ..], ds[r], ..)`)"""
    return [i for t in range(0, n, 16) for r in range(4) for fg in range(4) for i in [t + 4 * fg + r] if i < n]


def _chain(acc, w, x, order):
    """acc (..., m, D) fp32 += sum_i w[..., i, :]^T x[..., i, :] over i in `order`, one fused multiply-add per product: the product of two fp32 values is exact in
    float64, and the accumulator is rounded to fp32 after every term (tiles the kernels skip, and masked terms, add exact zeros: the full chain has the same value)"""
    for i in order:
        acc = (acc.double() + w[..., i, :, None].double() * x[..., i, None, :].double()).float()
    return acc


def emulate(qkv, dO, table, s: Shape, form: str, delta_from_rounded_o: bool = True, parts: bool = False):
    """-> dq (B, T, heads, D), dk, dv (B, T, kv, D), delta (B, heads, T), all fp32: the kernels' arithmetic up to summation order and __expf.
    delta_from_rounded_o = False takes delta from the un-rounded forward output instead (documentation of the 16-bit output's share; no kernel does that).
    parts (form "exact"): dK / dV as the PART kernels and attn_dkv_reduce_kernel form them -- one accumulation chain per q head, each share rotated back, the shares
    added in the order 0, 1, ... -- instead of one chain over all of the group's q heads."""
    B, T, heads, kv, D = s.B, s.T, s.heads, s.kv, s.D
    qd, kd, grp = heads * D, kv * D, heads // kv
    split = form == "split"
    o, lse = A.attention(qkv, heads, kv, D, table, s.lens, s.len_add, None, "split" if split else "f32")       # fp32 (B, T, heads, D), (B, heads, T)
    o_read = A.round_out(o).float() if delta_from_rounded_o else o                                              # hi + lo, added in fp32 as the dq kernels add them
    q = A._rotate(qkv[..., :qd].reshape(B, T, heads, D), table, 0, torch.float32).transpose(1, 2)              # (B, heads, T, D)
    k = A._rotate(qkv[..., qd:qd + kd].reshape(B, T, kv, D), table, 0, torch.float32).repeat_interleave(grp, dim=2).transpose(1, 2)
    v = qkv[..., qd + kd:qd + 2 * kd].reshape(B, T, kv, D).repeat_interleave(grp, dim=2).transpose(1, 2)
    g = dO.view(B, T, heads, D).transpose(1, 2)
    delta = (g * o_read.transpose(1, 2)).sum(-1)                                                                # (B, heads, T)
    klen = torch.tensor(key_lens(s))
    qi, kj = torch.arange(T)[:, None], torch.arange(T)[None, :]
    vis = (kj <= qi)[None, None] & (kj[None, None] < klen[:, None, None, None])                                 # the dq kernels' mask
    vis_kv = vis & (qi[None, None] < klen[:, None, None, None])                                                 # the dkv kernels': and qi < len
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32)
    if split:
        (qh, ql), (kh, kl), (vh, vl), (gh, gl) = A.split_bf16(q), A.split_bf16(k), A.split_bf16(v), A.split_bf16(g)
        sc = A._mm3(qh, ql, kh.transpose(-1, -2), kl.transpose(-1, -2))
        dp = A._mm3(gh, gl, vh.transpose(-1, -2), vl.transpose(-1, -2))
    else:
        # S and dP: a chain over head_dim per score, in the order MFMA4 feeds it (train_kernels.hip `MFMA4(sacc, kf, fq[c])`, `MFMA4(dpacc, vf, fdo[c])`: c ascending,
        # component x .. w, k = fg -> d = 16 c + 4 fg + e, the pattern of _mfma_order).  At peaked inputs (|S| ~ 200 before the scale) its rounding is what moves P.
        od = _mfma_order(D)
        sc = _chain(torch.zeros(B, heads, T, T), q.transpose(-1, -2), k.transpose(-1, -2), od)
        dp = _chain(torch.zeros(B, heads, T, T), g.transpose(-1, -2), v.transpose(-1, -2), od)
    e = torch.exp(sc * scale - lse[..., None])
    zero = torch.zeros((), dtype=torch.float32)
    p = torch.where(vis, e, zero)
    ds = p * (dp - delta[..., None]) * scale
    p_kv, ds_kv = torch.where(vis_kv, p, zero), torch.where(vis_kv, ds, zero)
    if split:
        (sh, sl), (ph2, pl2), (sh2, sl2) = A.split_bf16(ds), A.split_bf16(p_kv), A.split_bf16(ds_kv)
        dq = A._mm3(sh, sl, kh, kl)
        dk = A._mm3(sh2.transpose(-1, -2), sl2.transpose(-1, -2), qh, ql)
        dv = A._mm3(ph2.transpose(-1, -2), pl2.transpose(-1, -2), gh, gl)
        dk = dk.view(B, kv, grp, T, D).sum(2)
        dv = dv.view(B, kv, grp, T, D).sum(2)
        return _unrotate(dq.transpose(1, 2), table), _unrotate(dk.transpose(1, 2), table), dv.transpose(1, 2).contiguous(), delta
    order = _mfma_order(T)
    dq = _chain(torch.zeros(B, heads, T, D), ds.transpose(-1, -2), k, order)                                    # over the keys
    w_s, w_p = ds_kv.view(B, kv, grp, T, T), p_kv.view(B, kv, grp, T, T)                                        # [query i][key j]: the contraction index first
    xq, xg = q.view(B, kv, grp, T, D), g.view(B, kv, grp, T, D)
    if parts and grp > 1:
        sk = _chain(torch.zeros(B, kv, grp, T, D), w_s, xq, order)                                              # every q head's share
        sv = _chain(torch.zeros(B, kv, grp, T, D), w_p, xg, order)
        sk = _unrotate(sk.permute(0, 3, 1, 2, 4).reshape(B, T, heads, D), table).view(B, T, kv, grp, D)
        sv = sv.permute(0, 3, 1, 2, 4)
        dk, dv = sk[..., 0, :], sv[..., 0, :]
        for hh in range(1, grp):
            dk, dv = dk + sk[..., hh, :], dv + sv[..., hh, :]
        return _unrotate(dq.transpose(1, 2), table), dk.contiguous(), dv.contiguous(), delta
    dk, dv = torch.zeros(B, kv, T, D), torch.zeros(B, kv, T, D)
    for hh in range(grp):                                                                                       # one chain over the group's q heads
        dk = _chain(dk, w_s[:, :, hh], xq[:, :, hh], order)
        dv = _chain(dv, w_p[:, :, hh], xg[:, :, hh], order)
    return _unrotate(dq.transpose(1, 2), table), _unrotate(dk.transpose(1, 2), table), dv.transpose(1, 2).contiguous(), delta


def block_measure(got, ref, klens, unit=None) -> float:
    """got, ref (B, T, H, D) -> max over (batch, head) of max_{rows < klen} ||got - ref|| / RMS_{rows < klen} ||ref||; unit (B, H): the scale of a block whose
    reference vanishes identically (module docstring)"""
    got, ref = got.double(), ref.double()
    worst = 0.0
    for b, n in enumerate(klens):
        err = (got[b, :n] - ref[b, :n]).norm(dim=-1)                      # (n, H)
        rms = ref[b, :n].norm(dim=-1).pow(2).mean(dim=0).sqrt()           # (H)
        if bool((rms == 0).any()):
            assert unit is not None, "a reference block vanishes identically and no unit was given"
            rms = torch.where(rms == 0, unit[b].double(), rms)
        assert bool((rms > 0).all())
        worst = max(worst, float((err.max(dim=0).values / rms).max()))
    return worst


def delta_measure(got, ref, unit, klens) -> float:
    """got, ref (B, heads, T), unit (B, heads) = RMS_i ||dO_i|| ||o_i|| -> max |got - ref| / unit over the rows < klen"""
    worst = 0.0
    for b, n in enumerate(klens):
        worst = max(worst, float(((got[b, :, :n].double() - ref[b, :, :n].double()).abs().max(dim=-1).values / unit[b]).max()))
    return worst


def units(qkv, dO, o64, s: Shape):
    """-> delta's unit (B, heads) = RMS_{i < klen} ||dO_i|| ||o_i||, and the units of identically vanishing dq (B, heads) and dk (B, kv) blocks"""
    B, T, heads, kv, D = s.B, s.T, s.heads, s.kv, s.D
    qd, kd, grp = heads * D, kv * D, heads // kv
    scale = 1.0 / math.sqrt(D)
    x = qkv.double()
    qn = x[..., :qd].reshape(B, T, heads, D).norm(dim=-1)                 # rotation keeps the norms
    kn = x[..., qd:qd + kd].reshape(B, T, kv, D).norm(dim=-1)
    gn = dO.double().view(B, T, heads, D).norm(dim=-1) * o64.norm(dim=-1)  # (B, T, heads)
    du, uq, uk = torch.zeros(B, heads, dtype=torch.float64), torch.zeros(B, heads, dtype=torch.float64), torch.zeros(B, kv, dtype=torch.float64)
    for b, n in enumerate(key_lens(s)):
        du[b] = gn[b, :n].pow(2).mean(dim=0).sqrt()
        krms = kn[b, :n].pow(2).mean(dim=0).sqrt()                        # (kv)
        uq[b] = scale * du[b] * krms.repeat_interleave(grp)
        uk[b] = scale * (gn[b, :n] * qn[b, :n]).reshape(n, kv, grp).pow(2).mean(dim=(0, 2)).sqrt()
    return du, uq, uk


def measures(dq, dk, dv, delta, r) -> dict:
    """the four measures of one set of gradients against the float64 reference of r = reference(...)"""
    kl = key_lens(r["shape"])
    return {"dq": block_measure(dq, r["dq64"], kl, r["unit_dq"]), "dk": block_measure(dk, r["dk64"], kl, r["unit_dk"]),
            "dv": block_measure(dv, r["dv64"], kl), "delta": delta_measure(delta, r["delta64"], r["unit_delta"], kl)}


@functools.lru_cache(maxsize=None)
def reference(shape_name: str, form: str, parts: bool = False):
    """Everything the tests of one (shape, route) share, computed once: inputs, the float64 gradients and delta, the emulation and its own measures -- the GPU
    tests' bounds are twice these.  Treat the returned tensors as read-only."""
    s = SHAPE_BY_NAME[shape_name]
    qkv, dO, table = make_inputs(s)
    dq64, dk64, dv64, delta64, o64 = reference_f64(qkv, dO, table, s)
    du, uq, uk = units(qkv, dO, o64, s)
    r = {"shape": s, "qkv": qkv, "dO": dO, "table": table, "dq64": dq64, "dk64": dk64, "dv64": dv64, "delta64": delta64, "o64": o64,
         "unit_delta": du, "unit_dq": uq, "unit_dk": uk}
    r["emu"] = emulate(qkv, dO, table, s, form, parts=parts)
    r["emu_measures"] = measures(*r["emu"], r)
    return r
