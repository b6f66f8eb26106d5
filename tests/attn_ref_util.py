"""CPU references for the parity-mode decoder's fp32 forward attention (csrc/decoder_kernels.hip launch_attention_f32, csrc/attention_split.hip), shared by
tests/test_attention_reference_host.py (no GPU) and tests/test_gpu_decoder_ops.py.  TEST INFRASTRUCTURE ONLY.

The operator ([site] transformers/models/qwen2/modeling_qwen2.py:105-135, 150-234, restated in oracle/qwen2.py decoder_forward): causal GQA attention on packed
projections [q | k | v] with the rotate-half RoPE of a GIVEN fp32 (cos, sin) table, scale 1 / sqrt(D), key j visible to query i iff
j <= i and j < clamp(lens[b] + len_add, 1, T).  With a cached prefix the keys / values of positions < Np come from a [k | v] array and queries exist only for
positions >= Np.  Three forms of it:

  mode "f64"    the float64 reference (the fp32 table promoted to float64); lse = logsumexp of the scaled, masked scores
  mode "f32"    the same operator in torch fp32: what the exact-fp32 routes (attention_f32_mfma_kernel, attention_f32_kernel) compute up to summation order
  mode "split"  the split-bf16 route, from the header comment of attention_split.hip: every fp32 operand x is hi + lo (two bf16), every product is
                hi.hi + lo.hi + hi.lo (formed exactly, in float64, then rounded to fp32), scores, softmax and accumulation in fp32

and the output roundings of the kernels (round_out): hi = bf16(o), lo = bf16(o - hi), or for lo8 lo = e4m3((o - hi) * 256) / 256.

CASES are the shapes the GPU tests run; the host test checks the emulations' own worst-row error against CAPS at every one of them, so that the GPU tests'
bound (2 x that error) cannot hide a failure behind a loose emulation."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

THETA = 1e6
INPUT_SCALE = 0.8
PAD = 16          # ld, ldo, ldp are this many elements wider than the minimum
# the emulations' own worst query row against the float64 reference must stay under these (conditions, not tolerances)
CAPS = {"exact": 5e-6, "split": 1.2e-5, "lo8": 8e-5}


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    T: int
    heads: int
    kv: int
    D: int
    lens: Optional[Tuple[int, ...]] = None
    len_add: int = 0
    Np: int = 0
    lo8: bool = False
    use_split: bool = False
    lse: bool = False
    rope: bool = True

    @property
    def route(self) -> str:
        """the kernel launch_attention_f32 takes: "split" | "mfma" | "valu" """
        if self.D >= 64 and (self.lse or self.T >= 128) and not self.Np and not self.lo8 and self.use_split:
            return "split"
        return "mfma" if self.D >= 64 else "valu"

    @property
    def form(self) -> str:
        """which emulation (and cap) applies"""
        return "lo8" if self.lo8 else ("split" if self.route == "split" else "exact")

    def key_lens(self):
        if self.lens is None:
            return [self.T] * self.B
        return [max(1, min(int(l) + self.len_add, self.T)) for l in self.lens]


CASES = [
    # fp32-MFMA route, head_dim 64: two query blocks with a last block of 36 queries, two key chunks; a prompt of one token
    Case("mfma_d64_ragged", 3, 100, 4, 2, 64, lens=(100, 83, 1)),
    Case("mfma_d64_group7", 1, 65, 14, 2, 64),                           # 7 heads per group, ONE query in the second block
    Case("mfma_single_token", 2, 1, 4, 2, 64),
    Case("mfma_one_ragged_tile", 1, 17, 2, 2, 64),
    Case("mfma_no_table", 1, 17, 2, 2, 64, rope=False),                  # qkv taken as already rotated: the other staging branch
    Case("mfma_d128", 2, 70, 6, 2, 128, lens=(70, 33)),                  # KCH = 32: three chunks
    Case("mfma_T150_no_scratch", 2, 150, 4, 2, 64, lens=(150, 97)),      # T >= 128 without scratch: the shape class the suffix decoder runs
    Case("mfma_T127_scratch", 2, 127, 4, 2, 64, lens=(127, 64), use_split=True),   # below the threshold the scratch changes nothing
    Case("mfma_lse", 3, 100, 4, 2, 64, lens=(100, 83, 1), lse=True),     # row statistics of the fp32-MFMA kernel itself (no scratch)
    # split-bf16 route
    Case("split_T150", 2, 150, 4, 2, 64, lens=(150, 97), use_split=True),
    Case("split_T128", 2, 128, 4, 2, 64, lens=(128, 65), use_split=True),
    Case("split_no_grouping", 2, 200, 2, 2, 64, lens=(200, 183), use_split=True, lse=True),   # the per-head kernels
    Case("split_group9", 1, 130, 9, 1, 64, use_split=True),              # a group wider than a block holds: per-head kernels too
    Case("split_d128", 2, 130, 4, 2, 128, lens=(130, 77), use_split=True, lse=True),          # NT = 1
    Case("split_lse_below_threshold", 3, 100, 4, 2, 64, lens=(100, 83, 1), use_split=True, lse=True),
    # len_add: 45 / 60 keys, then 55 / 70 -> clamped to T
    Case("len_add_40", 2, 60, 4, 2, 64, lens=(5, 20), len_add=40),
    Case("len_add_50_clamps", 2, 60, 4, 2, 64, lens=(5, 20), len_add=50),
    # cached prefix
    Case("prefix_d64_np37", 2, 100, 4, 2, 64, Np=37),
    Case("prefix_d64_np64", 2, 100, 4, 2, 64, Np=64),
    Case("prefix_d128_np40", 2, 70, 6, 2, 128, Np=40),
    Case("prefix_ragged", 2, 100, 4, 2, 64, lens=(63, 20), len_add=37, Np=37),   # the engine's use: lens = text lengths, len_add = Np
    # hi + lo8 output
    Case("lo8_mfma", 2, 70, 4, 2, 64, lens=(70, 41), lo8=True),
    Case("lo8_valu", 2, 47, 4, 2, 32, lens=(47, 30), lo8=True),
    # VALU route (head_dim 32, rotation in place ahead of the kernel)
    Case("valu_d32", 2, 47, 4, 2, 32, lens=(47, 30)),
    Case("valu_d32_group7", 1, 100, 7, 1, 32),                           # 36 queries per block before levelling, 34 after: not a power of two
    Case("valu_d32_no_table", 2, 47, 4, 2, 32, lens=(47, 30), rope=False),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def rope_table(T: int, D: int, theta: float = THETA) -> torch.Tensor:
    """[T][D/2][2] fp32 (cos, sin): inv_freq = theta^(-2i/D) and angle = pos * inv_freq in fp32, as Qwen2RotaryEmbedding builds them"""
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous()


def make_inputs(c: Case, seed_extra: int = 0):
    """-> qkv (B, T - Np, (heads + 2 kv) D) fp32 un-rotated, pre (B, Np, 2 kv D) fp32 or None, table (T, D/2, 2) fp32 or None, full (B, T, ...) = the joint form"""
    g = torch.Generator().manual_seed(1000 * c.B + c.T + 7 * c.heads + c.D + 31 * c.Np + seed_extra)
    w = (c.heads + 2 * c.kv) * c.D
    full = torch.randn(c.B, c.T, w, generator=g) * INPUT_SCALE
    table = rope_table(c.T, c.D) if c.rope else None
    if c.Np:
        return full[:, c.Np:].contiguous(), full[:, :c.Np, c.heads * c.D:].contiguous(), table, full
    return full, None, table, full


def split_bf16(x: torch.Tensor):
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def _rotate(x, table, pos0, dt):
    """x (B, n, heads, D) at positions pos0 .. pos0 + n - 1; rotate-half: (a, b) -> (a cos - b sin, b cos + a sin)"""
    n, h = x.shape[1], x.shape[-1] // 2
    cs = table[pos0:pos0 + n].to(dt)
    co, si = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
    a, b = x[..., :h], x[..., h:]
    return torch.cat([a * co - b * si, b * co + a * si], dim=-1)


def _mm3(ah, al, bh, bl):
    """(ah + al) . (bh + bl) without the lo.lo term, every product exact (float64), the sum rounded to fp32"""
    ah, al, bh, bl = ah.double(), al.double(), bh.double(), bl.double()
    return (ah @ bh + al @ bh + ah @ bl).float()


def attention(qkv, heads, kv, D, table, lens=None, len_add=0, pre=None, mode="f64"):
    """qkv (B, Tq, (heads + 2 kv) D) fp32, the rows of positions Np .. T - 1; pre (B, Np, 2 kv D) or None (Np = 0).
    -> o (B, Tq, heads, D), lse (B, heads, Tq); float64 for mode "f64", fp32 otherwise (un-rounded: see round_out)."""
    B, Tq = qkv.shape[0], qkv.shape[1]
    Np = 0 if pre is None else pre.shape[1]
    T = Np + Tq
    qd, kd = heads * D, kv * D
    dt = torch.float64 if mode == "f64" else torch.float32
    q = qkv[..., :qd].reshape(B, Tq, heads, D).to(dt)
    k = qkv[..., qd:qd + kd].reshape(B, Tq, kv, D)
    v = qkv[..., qd + kd:qd + 2 * kd].reshape(B, Tq, kv, D)
    if pre is not None:
        k = torch.cat([pre[..., :kd].reshape(B, Np, kv, D), k], dim=1)
        v = torch.cat([pre[..., kd:2 * kd].reshape(B, Np, kv, D), v], dim=1)
    k, v = k.to(dt), v.to(dt)
    if table is not None:
        q, k = _rotate(q, table, Np, dt), _rotate(k, table, 0, dt)
    g = heads // kv
    q = q.transpose(1, 2)                                       # (B, heads, Tq, D)
    k = k.repeat_interleave(g, dim=2).transpose(1, 2)           # (B, heads, T, D)
    v = v.repeat_interleave(g, dim=2).transpose(1, 2)
    klen = torch.tensor([T] * B if lens is None else [max(1, min(int(l) + len_add, T)) for l in lens])
    qi, kj = torch.arange(Np, T)[:, None], torch.arange(T)[None, :]
    mask = (kj <= qi)[None, None] & (kj[None, None] < klen[:, None, None, None])   # (B, 1, Tq, T)
    if mode == "split":
        scale = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32)
        (qh, ql), (kh, kl), (vh, vl) = split_bf16(q), split_bf16(k), split_bf16(v)
        s = _mm3(qh, ql, kh.transpose(-1, -2), kl.transpose(-1, -2)) * scale
    else:
        s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    s = s.masked_fill(~mask, float("-inf"))
    if mode == "f64":
        lse = torch.logsumexp(s, dim=-1)
        return (torch.softmax(s, dim=-1) @ v).transpose(1, 2), lse
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    if mode == "split":
        ph, pl = split_bf16(p)
        o = _mm3(ph, pl, vh, vl) / l
    else:
        o = (p @ v) / l
    return o.transpose(1, 2), (m + torch.log(l)).squeeze(-1)


def round_out(o: torch.Tensor, lo8: bool = False) -> torch.Tensor:
    """fp32 o -> the value the kernels' two output halves decode to (float64): bf16 hi + bf16 lo, or bf16 hi + e4m3 lo (x 2^8)"""
    o = o.float()
    hi = o.to(torch.bfloat16).float()
    if lo8:
        lo = ((o - hi) * 256.0).to(torch.float8_e4m3fn).float() / 256.0
    else:
        lo = (o - hi).to(torch.bfloat16).float()
    return hi.double() + lo.double()


def row_errors(got, ref):
    """(B, Tq, heads, D) -> (B, Tq, heads) relative error of every query row over its head's D values"""
    got, ref = got.double(), ref.double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)


def valid_rows(c: Case) -> torch.Tensor:
    """(B, T - Np) bool: the query rows that are compared (positions < the batch entry's key length; rows past the prompt are never consumed)"""
    pos = torch.arange(c.Np, c.T)[None, :]
    return pos < torch.tensor(c.key_lens())[:, None]


def worst_row(got, ref, c: Case) -> float:
    e = row_errors(got, ref)
    return float(e[valid_rows(c)].max())


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """Everything the tests of one case share, computed once: inputs, the float64 reference and the matching emulation (decoded output, lse), and
    the emulation's own worst row / worst lse error -- the GPU tests' bound is twice these.  Treat the returned tensors as read-only."""
    c = CASE_BY_NAME[name]
    qkv, pre, table, full = make_inputs(c)
    o64, lse64 = attention(qkv, c.heads, c.kv, c.D, table, c.lens, c.len_add, pre, "f64")
    oe, lsee = attention(qkv, c.heads, c.kv, c.D, table, c.lens, c.len_add, pre, "split" if c.form == "split" else "f32")
    emu = round_out(oe, c.lo8)
    ok = valid_rows(c)
    lse_err = float((lsee.double() - lse64).abs().transpose(1, 2)[ok].max())
    return {"case": c, "qkv": qkv, "pre": pre, "table": table, "full": full, "o64": o64, "lse64": lse64, "emu": emu, "emu_raw": oe, "emu_lse": lsee,
            "emu_worst": worst_row(emu, o64, c), "raw_worst": worst_row(oe, o64, c), "emu_lse_err": lse_err}
