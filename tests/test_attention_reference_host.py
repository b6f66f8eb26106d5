"""CPU: the references tests/test_gpu_decoder_ops.py measures the decoder's fp32 forward attention against (tests/attn_ref_util.py).

  * the float64 reference is the oracle's attention (oracle/qwen2.py decoder_forward, pinned to the imported reference by the goldens);
  * its cached-prefix form equals the joint form on the rows >= Np;
  * the emulations of the kernels' arithmetic stay under attn_ref_util.CAPS at every shape the GPU tests use -- the GPU tests bound a kernel's worst query
    row by TWICE the matching emulation's, so these caps are what keeps a loose emulation from hiding a wrong kernel."""
import pytest
import torch

import attn_ref_util as A
from oracle import qwen2


def test_float64_reference_is_the_oracles_attention():
    """One decoder layer of oracle/qwen2.py wired so that only its attention acts: hidden = (heads + 2 kv) D, unit norm weight, q / k / v projections that
    select column ranges of the normed row, an o projection that writes the head outputs onto the first heads * D columns of the residual stream, a zero MLP.
    The embeddings are tiny (1e-4) and eps tinier, so forming the residual x + o and taking x off again costs o two more fp32 roundings and no
    cancellation.  GQA 6 q / 2 kv heads, ragged lengths.
    Tolerance: the oracle runs in fp32 -- rotation, a D = 64 dot product, softmax over <= 40 keys and the weighted sum each cost a few 2^-24 per element,
    some 1e-6 in a row's norm at worst (the fp32 form of this very reference measures 2.4e-7 .. 6e-7 at these scales): 2e-6 on the worst row."""
    B, T, heads, kv, D = 2, 40, 6, 2, 64
    qd, kd = heads * D, kv * D
    H = qd + 2 * kd
    cfg = qwen2.Qwen2Cfg(hidden=H, layers=1, heads=heads, kv_heads=kv, head_dim=D, inter=8, vocab=8, rope_theta=A.THETA, rms_eps=1e-30)
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(B, T, H, generator=g) * 1e-4
    lens = torch.tensor([T, 23])
    eye = torch.eye(H)
    pre = "model.layers.0."
    p = {pre + "input_layernorm.weight": torch.ones(H), pre + "post_attention_layernorm.weight": torch.ones(H), "model.norm.weight": torch.ones(H),
         pre + "self_attn.q_proj.weight": eye[:qd].clone(), pre + "self_attn.q_proj.bias": torch.zeros(qd),
         pre + "self_attn.k_proj.weight": eye[qd:qd + kd].clone(), pre + "self_attn.k_proj.bias": torch.zeros(kd),
         pre + "self_attn.v_proj.weight": eye[qd + kd:].clone(), pre + "self_attn.v_proj.bias": torch.zeros(kd),
         pre + "self_attn.o_proj.weight": eye[:, :qd].clone(),
         pre + "mlp.gate_proj.weight": torch.zeros(8, H), pre + "mlp.up_proj.weight": torch.zeros(8, H), pre + "mlp.down_proj.weight": torch.zeros(H, 8)}
    taps = {}
    qwen2.decoder_forward(p, emb, lens, cfg, taps=taps)
    o_oracle = (taps["layer0"] - emb)[..., :qd].reshape(B, T, heads, D)
    qkv = qwen2.rmsnorm(emb, torch.ones(H), cfg.rms_eps)                     # what the layer's projections select from
    cos, sin = qwen2.rope_tables(cfg, torch.arange(T))                       # the oracle's own fp32 table, handed to the reference
    table = torch.stack([cos[:, :D // 2], sin[:, :D // 2]], dim=-1)
    assert torch.equal(table, A.rope_table(T, D))                            # and the table the GPU tests build is that table
    o64, _ = A.attention(qkv, heads, kv, D, table, lens=lens, mode="f64")
    c = A.Case("oracle", B, T, heads, kv, D, lens=(T, 23))
    worst = A.worst_row(o_oracle, o64, c)
    print(f"oracle attention vs the float64 reference: worst row {worst:.2e}")
    assert worst <= 2e-6
    # the mask matters in this comparison: the reference with the second prompt's padding visible is far away on a row only IT changes (row 23 itself
    # is causal: rows < 23 never see key 23 anyway, so look at the last valid row under an off-by-one length)
    o_bad, _ = A.attention(qkv, heads, kv, D, table, lens=torch.tensor([T, 22]), mode="f64")
    assert float(A.row_errors(o_bad, o64)[1, 22].max()) > 1e-3


@pytest.mark.parametrize("name", [c.name for c in A.CASES if c.Np])
def test_prefix_form_of_the_reference_equals_the_joint_form(name):
    r = A.reference(name)
    c = r["case"]
    joint, lse_j = A.attention(r["full"], c.heads, c.kv, c.D, r["table"], c.lens, c.len_add, None, "f64")
    e = A.row_errors(r["o64"], joint[:, c.Np:])
    assert float(e.max()) <= 1e-14                                           # float64 rounding (another blocking of the same sums), every row
    assert float((r["lse64"] - lse_j[:, :, c.Np:]).abs().max()) <= 1e-13


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_emulations_stay_under_their_caps(name):
    r = A.reference(name)
    c = r["case"]
    print(f"[{name}] route {c.route}, form {c.form}: emulation worst row {r['emu_worst']:.2e} (before the output rounding {r['raw_worst']:.2e}), "
          f"lse abs {r['emu_lse_err']:.2e}; cap {A.CAPS[c.form]:.1e}")
    assert r["emu_worst"] <= A.CAPS[c.form]
    assert r["emu_worst"] > 0.0 and torch.isfinite(r["emu"]).all() and torch.isfinite(r["o64"]).all()


def test_the_cases_cross_the_edges_they_stand_for():
    """the routing the case list relies on, restated from launch_attention_f32 (a change there must be followed here)"""
    by = A.CASE_BY_NAME
    assert by["mfma_T150_no_scratch"].route == "mfma" and by["split_T150"].route == "split"
    assert by["mfma_T127_scratch"].route == "mfma" and by["split_T128"].route == "split"
    assert by["split_lse_below_threshold"].route == "split" and by["split_lse_below_threshold"].T < 128
    assert by["mfma_lse"].route == "mfma" and by["lo8_mfma"].route == "mfma" and by["lo8_valu"].route == "valu"
    assert all(c.route == "mfma" for c in A.CASES if c.Np)
    assert by["len_add_40"].key_lens() == [45, 60] and by["len_add_50_clamps"].key_lens() == [55, 60]
    assert by["prefix_ragged"].key_lens() == [100, 57]
    assert sum(c.lse and c.route == "split" for c in A.CASES) >= 3
