"""CPU references for the bf16 attention (csrc/attention.hip launch_attention: attention32_kernel, attention_kernel<D, MASKED>) and for the tower's attention
backward (csrc/tower_bwd_kernels.hip launch_tower_attn_bwd: tattn_dq_kernel, tattn_dkv_kernel), shared by tests/test_tower_attention_reference_host.py (no GPU)
and tests/test_gpu_tower_attention.py.  TEST INFRASTRUCTURE ONLY.

The forward operator: o = softmax(scale Q K^T + mask) V on bf16 q (B, T, heads, D), k, v (B, T, kv, D); key j visible to query i iff (not causal or j <= i) and
j < klen = clamp(lens[b] + len_add, 1, T) (lens None: T); q head h reads kv head h // (heads // kv).  The backward operator: the gradient of sum(dO o o) of the
UNMASKED head_dim-32 operator (kv = heads) with respect to packed rows [q | k | v], plus the row statistics the kernels keep, lse2 = log2 sum_j 2^(scale log2e s_ij)
and delta_i = sum_j P_ij dP_ij (= sum_d dO_id o_id in exact arithmetic).

  attention_f64 / backward_f64   the float64 references (backward: torch.autograd)
  emulate_forward                the two forward kernels' arithmetic, from their code: 64-key tiles in order, a running max per query, alpha rescales in fp32, P rounded
                                 to bf16 ahead of P.V (accumulated in fp32 per 32-key MFMA step), the output rounded to bf16, and
                                   attention32_kernel   max on the RAW scores, p = exp2(fma(s, c2, -m c2)), numerator AND row sum from the bf16-rounded p
                                   attention_kernel     scores scaled first (s c2), masked scores -1e30 with p forced to 0, the row sum from the UNROUNDED fp32 p
  emulate_backward               tattn_*: bf16 operands widened to fp16, fp32 scores and statistics tile by tile, delta from the same exponentials as the row sum,
                                 P and dS rounded to fp16 ahead of the second products (fp32 accumulation per 32-row MFMA step), outputs rounded to fp16 (IEEE: subnormals kept)

Measure (docs/kernels.md): per output tensor, batch entry and head the WORST valid row as ||got - ref|| over the RMS row norm of the same block of the float64
reference (attn_bwd_ref_util.block_measure); lse2 as an absolute difference; delta as |got - ref| / RMS_i(||dO_i|| ||o_i||).  A forward row is valid when it is < klen.
A block whose reference vanishes identically (T = 1: dQ = dK = 0) is measured against scale RMS_i(||dO_i|| ||o_i||) RMS ||k_j|| (for dK: ||q_i||).

CASES / BWD_CASES are what the GPU tests run; the host test holds the emulations' own measure under CAPS at every one of them, so the GPU bound (2 x the emulation
on the same inputs) cannot hide a wrong kernel behind a loose emulation.  The exact-bit inputs (selection_inputs, bwd_selection_inputs, constant_v_inputs) and their
checks live here too, so that the host test can run every check against the emulations."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from attn_bwd_ref_util import block_measure, delta_measure

PAD = 16              # every leading dimension is this many elements wider than its minimum
INPUT_SCALE = 0.8
PEAK = 3.0            # the peaked class multiplies q and k by this
SMALL_DO = 2.0 ** -10
LOG2E_F32 = 1.4426950408889634
FWD_KINDS = ("gauss", "peaked")
BWD_KINDS = ("gauss", "peaked", "small_dO")
# The emulations' own measure against float64 must stay under these: conditions, not tolerances.  The forward floor is the bf16 rounding of the output, the backward floor
# the fp16 rounding of P, dS and the output.  small_dO: dS ~ P (dP - delta) scale ~ 4e-3 x 3e-3 x 0.18 lies below fp16's smallest normal (6.1e-5), where the spacing is
# 2^-24 ABSOLUTE -- a relative 2^-24 / |dS| per term instead of 2^-11; dV = P^T dO has elements of ~2^-10 / sqrt(T), at T = 256 just at that edge: one cap for all three.
CAPS = {"forward": 5e-3, ("gauss", "dq"): 1.2e-3, ("gauss", "dk"): 1.2e-3, ("gauss", "dv"): 1.2e-3, ("peaked", "dq"): 2e-3, ("peaked", "dk"): 2e-3, ("peaked", "dv"): 2e-3,
        ("small_dO", "dq"): 1e-2, ("small_dO", "dk"): 1e-2, ("small_dO", "dv"): 1e-2}


def bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def h16(t):
    """fp32 -> the fp16 value pack_h2 stores (round to nearest even, subnormals kept, saturating)"""
    return t.clamp(-65504.0, 65504.0).to(torch.float16).to(torch.float32)


def f32_scale(D: int) -> float:
    """1 / sqrt(D) as the fp32 value the launchers receive"""
    return float(torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32))


def _c2(scale: float) -> torch.Tensor:
    """`p.scale * 1.4426950408889634f`: an fp32 product"""
    return torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------- forward
@dataclass(frozen=True)
class Case:
    name: str
    B: int
    T: int
    heads: int
    kv: int
    D: int
    causal: bool = False
    lens: Optional[Tuple[int, ...]] = None
    len_add: int = 0
    separate: bool = False        # q, k, v in three allocations with three different strides (otherwise one packed [q | k | v] buffer, PAD wider than its minimum)
    qk_gain: float = 1.0          # an extra factor on q and k in the Gaussian input class (the causal cases: see CASES)

    @property
    def masked(self) -> bool:
        """launch_attention: `const bool masked = causal || lens || (T & 63);`"""
        return bool(self.causal or self.lens is not None or (self.T & 63))

    @property
    def route(self) -> str:
        """the kernel launch_attention takes (product build: no FASTVLA_NO_ATTN32 switch): `if (D == 32 && !masked) attention32_kernel; else attention_kernel<D, masked>`"""
        if self.D == 32 and not self.masked:
            return "attention32_kernel"
        return f"attention_kernel<{self.D}, {'true' if self.masked else 'false'}>"

    @property
    def scale(self) -> float:
        return f32_scale(self.D)

    def key_lens(self):
        if self.lens is None:
            return [self.T] * self.B
        return [max(1, min(int(l) + self.len_add, self.T)) for l in self.lens]


# The causal cases carry qk_gain = 2.  With q and k at 0.8 a causal softmax is nearly uniform: query i averages i + 1 rows of v, so late rows shrink to ||v|| / sqrt(i) while
# the first rows keep ||v||, and the measure (worst row over the block's RMS row norm) reads the bf16 rounding of those first rows at twice its size -- the emulation alone
# measured 5.2e-3 .. 6.5e-3 over 8 seeds there, over the 5e-3 cap.  The cap stays; doubling q and k (score deviation 2.6 at head_dim 64) keeps the row norms within one
# block comparable (3.1e-3 .. 4.1e-3 over the same seeds).
CASES = [
    Case("a32_one_tile", 2, 64, 2, 2, 32),                                        # attention32_kernel, a single tile
    Case("a32_gqa", 1, 256, 4, 2, 32),                                            # its hk path, 4 tiles, xcd_remap over 16 blocks
    Case("a32_separate_buffers", 2, 128, 3, 3, 32, separate=True),
    Case("gen_d32_T49", 2, 49, 2, 2, 32),                                         # attention_kernel<32, true> through T & 63 only
    Case("gen_d32_T100", 1, 100, 4, 4, 32),                                       # two tiles, the last with 36 keys
    Case("gen_d32_T1", 2, 1, 2, 2, 32),                                           # one key
    Case("gen_d64_causal_ragged", 3, 100, 4, 2, 64, causal=True, lens=(100, 37, 1), qk_gain=2.0),   # the decoder's form
    Case("gen_d64_group7", 1, 65, 14, 2, 64, causal=True, qk_gain=2.0),                        # one query in the second block
    Case("gen_d128_causal", 2, 70, 4, 1, 128, causal=True, lens=(70, 33), qk_gain=2.0),        # DT = 8
    Case("gen_len_add_40", 2, 60, 4, 2, 64, causal=True, lens=(5, 20), len_add=40, qk_gain=2.0),
    Case("gen_len_add_50_clamps", 2, 60, 4, 2, 64, causal=True, lens=(5, 20), len_add=50, qk_gain=2.0),   # 55 / 70 -> clamped to T
    Case("gen_keymask_only", 2, 128, 2, 2, 64, lens=(128, 70)),                   # kend = len without the causal cut
    Case("gen_d64_unmasked", 1, 128, 2, 2, 64),                                   # the MASKED = false instances
    Case("gen_d128_unmasked", 1, 64, 2, 1, 128),
]
CASE_BY_NAME = {c.name: c for c in CASES}
# the kernel every case must reach (checked against Case.route on the CPU)
EXPECTED_ROUTE = {
    "a32_one_tile": "attention32_kernel", "a32_gqa": "attention32_kernel", "a32_separate_buffers": "attention32_kernel",
    "gen_d32_T49": "attention_kernel<32, true>", "gen_d32_T100": "attention_kernel<32, true>", "gen_d32_T1": "attention_kernel<32, true>",
    "gen_d64_causal_ragged": "attention_kernel<64, true>", "gen_d64_group7": "attention_kernel<64, true>", "gen_d128_causal": "attention_kernel<128, true>",
    "gen_len_add_40": "attention_kernel<64, true>", "gen_len_add_50_clamps": "attention_kernel<64, true>", "gen_keymask_only": "attention_kernel<64, true>",
    "gen_d64_unmasked": "attention_kernel<64, false>", "gen_d128_unmasked": "attention_kernel<128, false>",
}


def _seed(*v):
    return int(sum((i + 1) * 7919 * int(x) for i, x in enumerate(v)) % (2 ** 31 - 1))


def make_inputs(c: Case, kind: str):
    """-> q (B, T, heads, D), k, v (B, T, kv, D): fp32 holding bf16 values; kind "gauss" (x 0.8) or "peaked" (q and k x 3 on top)"""
    assert kind in FWD_KINDS
    g = torch.Generator().manual_seed(_seed(c.B, c.T, c.heads, c.kv, c.D, FWD_KINDS.index(kind)))
    q = torch.randn(c.B, c.T, c.heads, c.D, generator=g) * INPUT_SCALE
    k = torch.randn(c.B, c.T, c.kv, c.D, generator=g) * INPUT_SCALE
    v = torch.randn(c.B, c.T, c.kv, c.D, generator=g) * INPUT_SCALE
    if kind == "peaked":
        q, k = q * PEAK, k * PEAK
    gain = c.qk_gain if kind == "gauss" else 1.0
    return bf(q * gain), bf(k * gain), bf(v)


def visible(c: Case) -> torch.Tensor:
    """(B, 1, T, T) bool [b][.][query i][key j]"""
    qi, kj = torch.arange(c.T)[:, None], torch.arange(c.T)[None, :]
    vis = (kj < torch.tensor(c.key_lens())[:, None, None, None])
    if c.causal:
        vis = vis & (kj <= qi)[None, None]
    return vis.expand(c.B, 1, c.T, c.T)


def _heads_first(q, k, v, c: Case, dt):
    g = c.heads // c.kv
    return (q.to(dt).transpose(1, 2), k.to(dt).repeat_interleave(g, dim=2).transpose(1, 2), v.to(dt).repeat_interleave(g, dim=2).transpose(1, 2))


def attention_f64(q, k, v, c: Case) -> torch.Tensor:
    """-> o (B, T, heads, D) float64"""
    qq, kk, vv = _heads_first(q, k, v, c, torch.float64)
    s = (qq @ kk.transpose(-1, -2)) * c.scale
    s = s.masked_fill(~visible(c), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vv).transpose(1, 2)


def _pv_step(acc, p, x):
    """one MFMA step of the second product: acc (.., n, D) fp32 += p (.., n, 32 slots) . x (.., 32 slots, D), every product exact, the sum rounded to fp32 once.
    Slot s of p and row s of x must belong to the same key: that pairing is what the kernels' fragment order has to get right."""
    return (acc.double() + p.double() @ x.double()).float()


def emulate_forward(q, k, v, c: Case, kernel: Optional[str] = None, denominator_from_rounded_p: bool = True) -> torch.Tensor:
    """-> o (B, T, heads, D) fp32 holding the bf16 values the kernel stores.  kernel: "attention32_kernel" or anything else for attention_kernel (default: c.route).
    denominator_from_rounded_p = False sums the UN-rounded p in attention32_kernel's row sum (documentation of what the ones-operand MFMA buys; the kernel does not)."""
    a32 = (kernel or c.route) == "attention32_kernel"
    assert not (a32 and c.masked), "attention32_kernel has no masks"
    f32 = torch.float32
    qq, kk, vv = _heads_first(q, k, v, c, f32)
    B, H, T, D = qq.shape
    s_raw = (qq.double() @ kk.double().transpose(-1, -2)).float()                 # bf16 products are exact in fp32; the fp32 accumulation's order is not modelled
    vis = visible(c).expand(B, H, T, T)
    c2 = _c2(c.scale)
    o, l, m = torch.zeros(B, H, T, D), torch.zeros(B, H, T), torch.full((B, H, T), -1e30)
    for k0 in range(0, T, 64):
        k1 = min(k0 + 64, T)
        st, vt = s_raw[..., k0:k1], vis[..., k0:k1]
        if a32:
            m_new = torch.maximum(m, st.max(dim=-1).values)
            alpha = torch.exp2((m - m_new) * c2)                                   # the skipped rescale is alpha = exp2(0) = 1 exactly
            m = m_new
            mc = -m * c2
            p = torch.exp2((st.double() * c2.double() + mc.double()[..., None]).float())      # one fma
            pr = bf(p)
            lsrc = pr if denominator_from_rounded_p else p
            l = l * alpha
        else:
            sv = torch.where(vt, st * c2, torch.tensor(-1e30))
            m_new = torch.maximum(m, sv.max(dim=-1).values)
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(sv - m_new[..., None])
            p = torch.where(sv > -1e29, p, torch.zeros(()))
            l = l * alpha + p.sum(dim=-1)
            m = m_new
            pr = bf(p)
        o = o * alpha[..., None]
        for j0 in range(0, k1 - k0, 32):
            j1 = min(j0 + 32, k1 - k0)
            o = _pv_step(o, pr[..., j0:j1], vv[..., k0 + j0:k0 + j1, :])
            if a32:
                l = (l.double() + lsrc[..., j0:j1].double().sum(dim=-1)).float()  # the ones tile beside V^T: the same accumulation
    inv = torch.where(l > 0, 1.0 / l, torch.zeros(()))
    return bf(o * inv[..., None]).transpose(1, 2).contiguous()


def valid_rows(c: Case) -> torch.Tensor:
    """(B, T) bool: query rows < klen (rows past the prompt are never consumed)"""
    return torch.arange(c.T)[None, :] < torch.tensor(c.key_lens())[:, None]


def forward_measure(got, ref, c: Case) -> float:
    return block_measure(got, ref, c.key_lens())


@functools.lru_cache(maxsize=None)
def forward_reference(name: str, kind: str):
    """everything the tests of one (case, input class) share, computed once; read-only"""
    c = CASE_BY_NAME[name]
    q, k, v = make_inputs(c, kind)
    o64 = attention_f64(q, k, v, c)
    emu = emulate_forward(q, k, v, c)
    return {"case": c, "q": q, "k": k, "v": v, "o64": o64, "emu": emu, "emu_measure": forward_measure(emu, o64, c)}


# ---- exact selection: one-hot softmax rows ------------------------------------------------------------------------------------------------------------
def sign_keys(T: int, D: int) -> torch.Tensor:
    """(T, D) rows of +-1: the binary digits of j in columns 0 .. 9 (digit 1 -> -1), their parity in column 10, +1 elsewhere.  Two different rows differ in >= 2
    places, so k_a . k_b <= D - 4 for a != b"""
    assert T <= 1024 and D >= 11
    j = torch.arange(T)
    bits = torch.stack([(j >> b) & 1 for b in range(10)], dim=1)
    rows = torch.ones(T, D)
    rows[:, :10] = 1.0 - 2.0 * bits
    rows[:, 10] = 1.0 - 2.0 * (bits.sum(dim=1) & 1)
    return rows


def _maps(T: int, n: int, g: torch.Generator, limit=None):
    """n maps query -> key.  limit None: permutations of 0 .. T - 1, i -> (a i + c) mod T for a few a coprime to T, then random ones; otherwise limit (T) = the
    largest key each query may select: a random key in [0, limit[i]]"""
    out = []
    if limit is not None:
        for _ in range(n):
            out.append((torch.rand(T, generator=g) * (limit + 1).double()).long().clamp_max(limit))
        return out
    i = torch.arange(T)
    affine = [(a, c) for a, c in ((1, 0), (3, 5), (T - 1, 17), (11, 63), (29, 1)) if math.gcd(a, T) == 1]
    for n_ in range(n):
        if n_ % 3 == 2 or not affine:
            out.append(torch.randperm(T, generator=g))
        else:
            a, c = affine[(n_ - n_ // 3) % len(affine)]
            out.append((a * i + c) % T)
    return out


def selection_inputs(c: Case):
    """-> q, k, v as make_inputs and pi (B, heads, T): query i of (b, h) scores 512 D on key pi[b, h, i] and <= 512 (D - 4) on every other one, so in the log2
    domain the others lie >= 2048 scale log2e >= 260 below the maximum: their exponentials are exactly 0 in fp32, P is one-hot and the row sum exactly 1.
    Expected output row i: v[b, pi[b, h, i], h // group] bit for bit."""
    g = torch.Generator().manual_seed(_seed(c.B, c.T, c.heads, c.D, 99))
    keys = sign_keys(c.T, c.D)
    k = keys[None, :, None, :].expand(c.B, c.T, c.kv, c.D).contiguous()
    v = bf(torch.randn(c.B, c.T, c.kv, c.D, generator=g) * 2.0)
    pi = torch.zeros(c.B, c.heads, c.T, dtype=torch.long)
    i = torch.arange(c.T)
    for b, n in enumerate(c.key_lens()):
        limit = None
        if c.masked and (c.causal or n < c.T):
            limit = torch.minimum(i, torch.tensor(n - 1)) if c.causal else torch.full((c.T,), n - 1)
        for h, mp in enumerate(_maps(c.T, c.heads, g, limit)):
            pi[b, h] = mp
    q = 512.0 * keys[pi].transpose(1, 2).contiguous()                              # (B, T, heads, D)
    assert 2048.0 * c.scale * LOG2E_F32 >= 260.0
    return q, k, v, pi


def selection_expected(v, pi, c: Case) -> torch.Tensor:
    """(B, T, heads, D): v row pi[b, h, i] of kv head h // group"""
    grp = c.heads // c.kv
    out = torch.empty(c.B, c.T, c.heads, c.D)
    for b in range(c.B):
        for h in range(c.heads):
            out[b, :, h] = v[b, pi[b, h], h // grp]
    return out


# ---- constant V -------------------------------------------------------------------------------------------------------------------------------------
CONST_V_VARIANTS = ("plain", "plateau", "first_tile_max", "rising_max")


def constant_v_variants(c: Case, kind: str):
    """the variants run at (case, input class): the planted ones once per case (they replace q and k), the two tile variants where attention32_kernel has several tiles"""
    if kind != "gauss":
        return ("plain",)
    return CONST_V_VARIANTS if (c.route == "attention32_kernel" and c.T > 64) else ("plain", "plateau")


def constant_v_inputs(c: Case, kind: str, variant: str = "plain"):
    """-> q, k, v, cd (B, kv, D): v[b, j, hk, d] = cd[b, hk, d] for every key j.  Variants plant column 0 of q and k (the last two: Gaussian class, T > 64) so that
    "plateau" (any case): q_i = (x_i, 0, ..), column 0 of k = 1 at key 0 and 1/2 elsewhere -- the visible keys j >= 1 of query i all carry the SAME p = 2^(-x_i c2 / 2), so its
    bf16 rounding error does not average out in the row sum: sum(p) and sum(bf16(p)) differ by up to 2^-8 relative, which is what it takes to move a bf16 output
    (Gaussian rows spread over many keys never get there); x_i varies from query to query, and with it the rounding error of p;
    "first_tile_max": every query's global maximum is key 0 -- no later tile moves a maximum, attention32_kernel skips every rescale after the first tile;
    "rising_max": key 64 t scores 64 (t + 1) + noise -- every query's maximum rises strictly tile by tile, every rescale is taken."""
    assert variant in CONST_V_VARIANTS
    q, k, _ = make_inputs(c, kind)
    g = torch.Generator().manual_seed(_seed(c.B, c.kv, c.D, 5))
    cd = bf(torch.randn(c.B, c.kv, c.D, generator=g) * 1.5)
    v = cd[:, None].expand(c.B, c.T, c.kv, c.D).contiguous()
    if variant == "plateau":
        x = bf(4.0 + 8.0 * torch.rand(c.B, c.T, c.heads, generator=g))
        q, k = torch.zeros_like(q), k.clone()
        q[..., 0] = x
        k[..., 0] = 0.5
        k[:, 0, :, 0] = 1.0
    elif variant != "plain":
        assert kind == "gauss" and c.T > 64
        q, k = q.clone(), k.clone()
        q[..., 0] = 8.0
        k[..., 0] = 0.0
        if variant == "first_tile_max":
            k[:, 0, :, 0] = 8.0
        else:
            for t in range(c.T // 64):
                k[:, 64 * t, :, 0] = 8.0 * (t + 1)
    return q, k, v, cd


def tile_maxima(q, k, c: Case) -> torch.Tensor:
    """(B, heads, T, tiles) float64: every query's largest raw score in each 64-key tile (T % 64 == 0)"""
    qq, kk, _ = _heads_first(q, k, k, c, torch.float64)
    s = qq @ kk.transpose(-1, -2)
    return s.view(c.B, c.heads, c.T, c.T // 64, 64).max(dim=-1).values


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """the spacing of bf16 just above |x| (x a normal bf16 value)"""
    _, e = torch.frexp(x.abs().double())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


def constant_v_deviation(got, cd, c: Case):
    """got (B, T, heads, D) -> (|got - c_d| in bf16 ulps of c_d (B, T, heads, D), over the valid rows the number of elements off, the number compared)"""
    grp = c.heads // c.kv
    want = cd.repeat_interleave(grp, dim=1)[:, None].expand(c.B, c.T, c.heads, c.D)
    dev = (got.double() - want.double()).abs() / bf16_ulp(want)
    ok = valid_rows(c)[:, :, None, None].expand_as(dev)
    return dev, int((dev[ok] != 0).sum()), int(ok.sum())


# --------------------------------------------------------------------------------------------------------------------------------------------- backward
@dataclass(frozen=True)
class BwdCase:
    B: int
    T: int
    heads: int

    @property
    def name(self) -> str:
        return f"b{self.B}_T{self.T}_h{self.heads}"

    @property
    def C(self) -> int:
        return 32 * self.heads

    @property
    def scale(self) -> float:
        return f32_scale(32)


BWD_CASES = [BwdCase(2, 64, 2), BwdCase(1, 256, 4), BwdCase(2, 100, 3), BwdCase(1, 49, 2), BwdCase(1, 1, 1), BwdCase(2, 130, 1)]   # T = 130: two keys in the last tile
BWD_BY_NAME = {c.name: c for c in BWD_CASES}


def make_bwd_inputs(c: BwdCase, kind: str):
    """-> qkv (B, T, 3 C) fp32 holding bf16 values, dO (B, T, C) fp32 holding fp16 values (unit scale; "small_dO": x 2^-10, where dS is an fp16 subnormal)"""
    assert kind in BWD_KINDS
    g = torch.Generator().manual_seed(_seed(c.B, c.T, c.heads, 3, BWD_KINDS.index(kind)))
    qkv = torch.randn(c.B, c.T, 3 * c.C, generator=g) * INPUT_SCALE
    if kind == "peaked":
        qkv[..., :2 * c.C] *= PEAK
    dO = torch.randn(c.B, c.T, c.C, generator=g)
    if kind == "small_dO":
        dO = dO * SMALL_DO
    return bf(qkv), h16(dO)


def _split_heads(qkv, c: BwdCase, dt):
    """(B, T, 3 C) -> q, k, v (B, heads, T, 32)"""
    x = qkv.to(dt).view(c.B, c.T, 3, c.heads, 32)
    return x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)


def backward_f64(qkv, dO, c: BwdCase):
    """float64 autograd -> dq, dk, dv (B, T, heads, 32), lse2, delta (B, heads, T), o (B, T, heads, 32)"""
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = _split_heads(x, c, torch.float64)
    s = (q @ k.transpose(-1, -2)) * c.scale
    o = torch.softmax(s, dim=-1) @ v                                               # (B, heads, T, 32)
    w = dO.double().view(c.B, c.T, c.heads, 32).transpose(1, 2)
    (w * o).sum().backward()
    gr = x.grad.view(c.B, c.T, 3, c.heads, 32)
    lse2 = torch.logsumexp(s.detach(), dim=-1) / math.log(2.0)
    dp = w @ v.detach().transpose(-1, -2)
    delta = (torch.softmax(s.detach(), dim=-1) * dp).sum(dim=-1)
    return gr[:, :, 0], gr[:, :, 1], gr[:, :, 2], lse2, delta, o.detach().transpose(1, 2)


def emulate_backward(qkv, dO, c: BwdCase, delta_from_exponentials: bool = True):
    """-> dq, dk, dv (B, T, heads, 32) fp32 holding fp16 values, lse2, delta (B, heads, T) fp32.
    delta_from_exponentials = False takes delta = sum_d dO o from the forward's bf16-ROUNDED output instead (the textbook shortcut the kernels avoid)."""
    f32 = torch.float32
    q, k, v = (h16(t) for t in _split_heads(qkv, c, f32))                          # bf16 -> fp16 on the way into LDS / registers
    g = dO.view(c.B, c.T, c.heads, 32).transpose(1, 2)
    B, H, T = c.B, c.heads, c.T
    scale = torch.tensor(c.scale, dtype=f32)
    c2 = _c2(c.scale)
    sv = (q.double() @ k.double().transpose(-1, -2)).float() * c2                   # [query i][key j], log2 domain
    dp = (g.double() @ v.double().transpose(-1, -2)).float()                       # dP_ij = dO_i . v_j
    m, l, d = torch.full((B, H, T), -1e30), torch.zeros(B, H, T), torch.zeros(B, H, T)
    for k0 in range(0, T, 64):                                                     # pass 1 of tattn_dq_kernel
        k1 = min(k0 + 64, T)
        st = sv[..., k0:k1]
        m_new = torch.maximum(m, st.max(dim=-1).values)
        e = torch.exp2(st - m_new[..., None])
        alpha = torch.exp2(m - m_new)
        l = l * alpha + e.sum(dim=-1)
        d = d * alpha + (e * dp[..., k0:k1]).sum(dim=-1)
        m = m_new
    lse2 = m + torch.log2(l)
    delta = d / l
    if not delta_from_exponentials:
        o = bf((torch.softmax(sv.double() * math.log(2.0), dim=-1) @ v.double()).float())
        delta = (g * o).sum(dim=-1)
    p = torch.exp2(sv - lse2[..., None])
    ds = p * (dp - delta[..., None]) * scale
    p16, ds16 = h16(p), h16(ds)
    dq, dk, dv = torch.zeros(B, H, T, 32), torch.zeros(B, H, T, 32), torch.zeros(B, H, T, 32)
    for r0 in range(0, T, 32):                                                     # one MFMA step = 32 keys (dq) / 32 queries (dk, dv)
        r1 = min(r0 + 32, T)
        dq = _pv_step(dq, ds16[..., :, r0:r1], k[..., r0:r1, :])
        dk = _pv_step(dk, ds16[..., r0:r1, :].transpose(-1, -2), q[..., r0:r1, :])
        dv = _pv_step(dv, p16[..., r0:r1, :].transpose(-1, -2), g[..., r0:r1, :])
    return h16(dq).transpose(1, 2), h16(dk).transpose(1, 2), h16(dv).transpose(1, 2), lse2, delta


def backward_units(qkv, dO, o64, c: BwdCase):
    """-> delta's unit (B, heads) = RMS_i ||dO_i|| ||o_i||, and the units of identically vanishing dq / dk blocks (B, heads)"""
    q, k, _ = _split_heads(qkv, c, torch.float64)
    gn = dO.double().view(c.B, c.T, c.heads, 32).norm(dim=-1) * o64.norm(dim=-1)    # (B, T, heads)
    du = gn.pow(2).mean(dim=1).sqrt()
    uq = c.scale * du * k.norm(dim=-1).pow(2).mean(dim=-1).sqrt()
    uk = c.scale * (gn * q.norm(dim=-1).transpose(1, 2)).pow(2).mean(dim=1).sqrt()
    return du, uq, uk


def backward_measures(dq, dk, dv, lse2, delta, r) -> dict:
    c = r["case"]
    kl = [c.T] * c.B
    return {"dq": block_measure(dq, r["dq64"], kl, r["unit_dq"]), "dk": block_measure(dk, r["dk64"], kl, r["unit_dk"]), "dv": block_measure(dv, r["dv64"], kl),
            "lse2": float((lse2.double() - r["lse2_64"]).abs().max()), "delta": delta_measure(delta, r["delta64"], r["unit_delta"], kl)}


@functools.lru_cache(maxsize=None)
def backward_reference(name: str, kind: str):
    """everything the tests of one (case, input class) share, computed once; read-only"""
    c = BWD_BY_NAME[name]
    qkv, dO = make_bwd_inputs(c, kind)
    dq64, dk64, dv64, lse64, delta64, o64 = backward_f64(qkv, dO, c)
    du, uq, uk = backward_units(qkv, dO, o64, c)
    r = {"case": c, "qkv": qkv, "dO": dO, "dq64": dq64, "dk64": dk64, "dv64": dv64, "lse2_64": lse64, "delta64": delta64, "o64": o64,
         "unit_delta": du, "unit_dq": uq, "unit_dk": uk}
    r["emu"] = emulate_backward(qkv, dO, c)
    r["emu_measures"] = backward_measures(*r["emu"], r)
    return r


def bwd_selection_inputs(c: BwdCase, many_to_one: bool = False):
    """-> qkv (B, T, 3 C), dO (B, T, C), pi (B, heads, T).  q, k as selection_inputs (a permutation per (b, h), or with many_to_one a random map); v and dO are
    multiples of 1/16 below 8 in magnitude (exact in bf16 and fp16, and every sum of their products exact in fp32).  P is one-hot in fp16, so
    dV row j = sum of the dO rows i with pi(i) = j, lse2 = the selected score in the log2 domain, delta_i = dO_i . v_pi(i), and dP_i,pi(i) - delta_i = 0: dQ = dK = 0."""
    g = torch.Generator().manual_seed(_seed(c.B, c.T, c.heads, 77, int(many_to_one)))
    keys = sign_keys(c.T, 32)
    limit = torch.full((c.T,), c.T - 1) if many_to_one else None
    pi = torch.stack([torch.stack(_maps(c.T, c.heads, g, limit)) for _ in range(c.B)])             # (B, heads, T)
    q = 512.0 * keys[pi].transpose(1, 2)                                                          # (B, T, heads, 32)
    k = keys[None, :, None, :].expand(c.B, c.T, c.heads, 32)
    v = torch.randint(-127, 128, (c.B, c.T, c.heads, 32), generator=g).float() / 16.0
    dO = torch.randint(-127, 128, (c.B, c.T, c.heads, 32), generator=g).float() / 16.0
    qkv = torch.stack([q, k, v], dim=2).reshape(c.B, c.T, 3 * c.C).contiguous()
    return qkv, dO.reshape(c.B, c.T, c.C).contiguous(), pi


def bwd_selection_expected(qkv, dO, pi, c: BwdCase):
    """-> dv (B, T, heads, 32), lse2, delta (B, heads, T), all exact in fp32"""
    v = qkv.view(c.B, c.T, 3, c.heads, 32)[:, :, 2]
    g = dO.view(c.B, c.T, c.heads, 32)
    dv = torch.zeros(c.B, c.T, c.heads, 32)
    delta = torch.zeros(c.B, c.heads, c.T)
    for b in range(c.B):
        for h in range(c.heads):
            dv[b, :, h].index_add_(0, pi[b, h], g[b, :, h])
            delta[b, h] = (g[b, :, h] * v[b, pi[b, h], h]).sum(dim=-1)
    lse2 = (torch.tensor(512.0 * 32.0) * _c2(c.scale)).expand(c.B, c.heads, c.T)
    return dv, lse2, delta
