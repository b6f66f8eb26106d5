// ops_api.hip -- op-level C entry points (include/fastvla_hip_testops.h: TEST-ONLY, built into vla-from-fastvlm_amd/testops/libfastvla_hip_testops.so, not into the product library): one kernel each, so the
// parity tests can check every kernel of the path against the oracle on its own.  No engine state is involved.
#include <cmath>
#include <cstdio>
#include <vector>

#include "kernels.h"

extern "C" {

int fv_op_gemm(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const float* scale,
               const void* res, int ldr, void* out, int ldo, int epilogue, fv_stream s) {
  fv::GemmArgs g{static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(W), M, N, K, bias, scale, res, ldr, out, ldo, epilogue};
  return fv::launch_gemm(g, static_cast<hipStream_t>(s));
}
int fv_op_gemm_ksplit(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const void* res, int ldr,
                      void* out, int ldo, int epilogue, fv_stream s) {
  fv::GemmArgs g{static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(W), M, N, K, bias, nullptr, res, ldr, out, ldo, epilogue};
  g.ksplit = true;
  return fv::launch_gemm(g, static_cast<hipStream_t>(s));
}
int fv_op_gemm_splitk(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const void* res, int ldr,
                      void* out, int ldo, int epilogue, int ksplit, void* ws, size_t ws_bytes, fv_stream s) {
  fv::GemmArgs g{static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(W), M, N, K, bias, nullptr, res, ldr, out, ldo, epilogue};
  g.ksplit = ksplit != 0;
  g.splitk_ws = static_cast<float*>(ws);
  g.splitk_bytes = ws_bytes;
  return fv::launch_gemm(g, static_cast<hipStream_t>(s));
}
// fv_op_gemm_splitk plus what the decoder sets on its launches: the layer scale (FV_EPI_LS_RES behind K ranges), GemmArgs::few_rows (0: the training path's
// setting) and the RMSNorm that follows the fp32 output (fused into the split-K reducer where K ranges are taken, a separate launch otherwise)
int fv_op_gemm_norm(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const float* scale, const void* res, int ldr, void* out,
                    int ldo, int epilogue, int ksplit, void* ws, size_t ws_bytes, int few_rows, const float* norm_w, void* norm_y, void* norm_ylo, int norm_ld,
                    float norm_eps, fv_stream s) {
  fv::GemmArgs g{static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(W), M, N, K, bias, scale, res, ldr, out, ldo, epilogue};
  g.ksplit = ksplit != 0;
  g.splitk_ws = static_cast<float*>(ws);
  g.splitk_bytes = ws_bytes;
  g.few_rows = few_rows;
  g.norm_w = norm_w; g.norm_y = static_cast<bf16_t*>(norm_y); g.norm_ylo = static_cast<bf16_t*>(norm_ylo); g.norm_ld = norm_ld; g.norm_eps = norm_eps;
  return fv::launch_gemm(g, static_cast<hipStream_t>(s));
}
// what launch_gemm would do with the problem on a device of `cus` CUs: plan_gemm's answer, no launch.  The planner reads no memory, so the operands that are
// marked present are one aligned dummy.  Returns the number of launches written to `out` (1, or 2 with the tail cut off) or the refusal's code (negative).
int fv_op_gemm_plan(int M, int N, int K, int lda, int ldw, int ldo, int ldr, int epilogue, int ksplit, int f16, int tn, int few_rows, int cus, size_t ws_bytes,
                    int has_bias, int has_scale, int has_res, int has_stash, int has_norm, int has_w8, fv_gemm_plan_launch* out) {
  alignas(16) static float mem[4];
  const auto at = [](int present) { return present ? mem : nullptr; };
  fv::GemmArgs g{reinterpret_cast<const bf16_t*>(mem), lda, reinterpret_cast<const bf16_t*>(mem), M, N, K, at(has_bias), at(has_scale), at(has_res), ldr, mem, ldo, epilogue, ksplit};
  g.f16 = f16; g.tn = tn; g.ldw = ldw; g.few_rows = few_rows;
  g.splitk_ws = at(ws_bytes != 0); g.splitk_bytes = ws_bytes;
  g.stash = at(has_stash); g.W8 = at(has_w8);
  g.norm_w = at(has_norm); g.norm_y = reinterpret_cast<bf16_t*>(at(has_norm)); g.norm_ld = N;
  fv::GemmPlan plan;
  const int rc = fv::plan_gemm(g, cus, plan);
  if (rc != FV_OK) return rc;
  for (int i = 0; i < plan.n; ++i) {
    const fv::GemmLaunch& l = plan.launch[i];
    fv_gemm_plan_launch& o = out[i];
    snprintf(o.kernel, sizeof(o.kernel), "%s", fv::gemm_kernel_name(l.kernel));
    snprintf(o.reducer, sizeof(o.reducer), "%s", fv::gemm_reducer_name(l.reducer));
    o.tile = l.tile; o.tiles_m = l.tiles_m; o.group_m = l.group_m; o.splits = l.splits; o.npad = l.npad; o.grid = l.grid; o.norm = l.norm; o.c0 = l.c0; o.c1 = l.c1;
  }
  return plan.n;
}

int fv_op_gemm_tn(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int f16, const float* bias, void* out, int ldo, void* ws,
                  size_t ws_bytes, fv_stream s) {
  fv::GemmArgs g{static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(W), M, N, K, bias, nullptr, nullptr, 0, out, ldo, FV_EPI_F32};
  g.tn = 1; g.ldw = ldw; g.f16 = f16 != 0;
  g.splitk_ws = static_cast<float*>(ws);
  g.splitk_bytes = ws_bytes;
  return fv::launch_gemm(g, static_cast<hipStream_t>(s));
}

int fv_op_gemm_lo8(const void* A, int lda, const void* W, const void* W8, int M, int N, int K, const float* bias, const void* res, int ldr, void* out,
                   int ldo, int epilogue, void* ws, size_t ws_bytes, fv_stream s) {
  fv::GemmArgs g{static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(W), M, N, K, bias, nullptr, res, ldr, out, ldo, epilogue};
  g.ksplit = 2;
  g.W8 = W8;
  g.splitk_ws = static_cast<float*>(ws);
  g.splitk_bytes = ws_bytes;
  return fv::launch_gemm(g, static_cast<hipStream_t>(s));
}
int fv_op_lo8_pack(const float* x, void* a_out, int lda, const void* W, void* w8_out, int M, int K, int N, fv_stream s) {
  // x (M, K) f32 -> the hi + lo8 operand rows (lda bf16 units each: K bf16, then at byte 2K the K fp8 remainders); W (N, K) bf16 -> W8
  int rc = FV_OK;
  if (x && a_out) {
    // RMSNorm with unit weights would rescale: use the plain split of the training glue for hi, then its remainders as fp8
    rc = fv::launch_split_rows(x, K, static_cast<bf16_t*>(a_out), lda, 0, M, K, static_cast<hipStream_t>(s));
    if (rc == FV_OK) rc = fv::launch_lo8_rows(x, K, static_cast<bf16_t*>(a_out), lda, M, K, static_cast<hipStream_t>(s));
  }
  if (rc == FV_OK && W && w8_out) rc = fv::launch_bf16_to_w8(static_cast<const bf16_t*>(W), w8_out, (size_t)N, K, static_cast<hipStream_t>(s));
  return rc;
}

int fv_op_gemm_f16(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const void* res, int ldr, void* out,
                   int ldo, int epilogue, void* ws, size_t ws_bytes, fv_stream s) {
  fv::GemmArgs g{static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(W), M, N, K, bias, nullptr, res, ldr, out, ldo, epilogue};
  g.f16 = 1;
  g.splitk_ws = static_cast<float*>(ws);
  g.splitk_bytes = ws_bytes;
  return fv::launch_gemm(g, static_cast<hipStream_t>(s));
}

int fv_op_dwconv(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C, int k,
                 int stride, int mult, int gelu, fv_stream s) {
  return fv::launch_dwconv(static_cast<const bf16_t*>(x), w, bias, static_cast<bf16_t*>(y), B, H, W, C, k, stride, mult, gelu, static_cast<hipStream_t>(s));
}

int fv_op_stem_conv(const void* pix, const float* w, const float* bias, void* y, int B, int S, int Cout, fv_stream s) {
  return fv::launch_stem_conv(static_cast<const bf16_t*>(pix), w, bias, static_cast<bf16_t*>(y), B, S, Cout, static_cast<hipStream_t>(s));
}

int fv_op_stem_mfma(const void* pix, const void* wp, const float* bias, void* y, int B, int S, int Cout, fv_stream s) {
  return fv::launch_stem_mfma(static_cast<const bf16_t*>(pix), static_cast<const bf16_t*>(wp), bias, static_cast<bf16_t*>(y), B, S, Cout, static_cast<hipStream_t>(s));
}
int fv_op_stem_fused(const void* pix, const void* wp, const float* b1, const float* w2, const float* b2, void* y, int B, int S, int Cout,
                     fv_stream s) {
  return fv::launch_stem_fused(static_cast<const bf16_t*>(pix), static_cast<const bf16_t*>(wp), b1, w2, b2, static_cast<bf16_t*>(y), B, S, Cout,
                               static_cast<hipStream_t>(s));
}

int fv_op_stem_fused_images(const void* img, int dtype, int B, int C, int Hin, int Win, float pad_value, int resize_with_padding, const void* wp,
                            const float* b1, const float* w2, const float* b2, void* y, int S, int Cout, fv_stream s) {
  return fv::launch_stem_fused_lb(img, dtype, B, C, Hin, Win, pad_value, resize_with_padding, static_cast<const bf16_t*>(wp), b1, w2, b2,
                                  static_cast<bf16_t*>(y), S, Cout, static_cast<hipStream_t>(s));
}

int fv_op_layernorm_rows(const void* x, const float* w, const float* b, void* y, int rows, int C, float eps, fv_stream s) {
  return fv::launch_layernorm_rows(static_cast<const bf16_t*>(x), w, b, static_cast<bf16_t*>(y), rows, C, eps, static_cast<hipStream_t>(s));
}

int fv_op_attention(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, void* out, int ldo, int B,
                    int T, int heads, int kv_heads, int D, int causal, const int32_t* lens, float scale, fv_stream s) {
  return fv::launch_attention(static_cast<const bf16_t*>(q), static_cast<const bf16_t*>(k), static_cast<const bf16_t*>(v), ldq, ldk,
                              ldv, static_cast<bf16_t*>(out), ldo, B, T, heads, kv_heads, D, causal, lens, 0, scale, static_cast<hipStream_t>(s));
}

int fv_op_attention_bf16(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, void* out, int ldo, int B, int T, int heads, int kv_heads, int D,
                         int causal, const int32_t* lens, int len_add, float scale, fv_stream s) {
  return fv::launch_attention(static_cast<const bf16_t*>(q), static_cast<const bf16_t*>(k), static_cast<const bf16_t*>(v), ldq, ldk, ldv, static_cast<bf16_t*>(out), ldo,
                              B, T, heads, kv_heads, D, causal, lens, len_add, scale, static_cast<hipStream_t>(s));
}

int fv_op_tower_attention_bwd(const void* qkv, int ld, const void* dO, int lddo, void* dqkv, int ldd, float* stats, int B, int T, int heads, float scale, fv_stream s) {
  return fv::launch_tower_attn_bwd(static_cast<const bf16_t*>(qkv), ld, static_cast<const bf16_t*>(dO), lddo, static_cast<bf16_t*>(dqkv), ldd, stats, B, T, heads, scale,
                                   static_cast<hipStream_t>(s));
}

int fv_op_rmsnorm(const float* x, const float* w, void* y_bf16, int rows, int H, float eps, fv_stream s) {
  return fv::launch_rmsnorm(x, w, static_cast<bf16_t*>(y_bf16), nullptr, H, rows, H, eps, static_cast<hipStream_t>(s));
}

int fv_op_rope(void* qkv, int ld, int rows, int T, int heads, int kv_heads, int D, float theta, fv_stream s) {
  if (T <= 0 || D <= 0 || D % 16) return fv_fail(FV_ERR_ARG, "rope: bad T/D");
  std::vector<float> cs((size_t)T * D);
  fv::rope_table_host(cs.data(), T, D, theta);
  float2* tab = nullptr;
  FV_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&tab), cs.size() * 4));
  hipError_t e = hipMemcpy(tab, cs.data(), cs.size() * 4, hipMemcpyHostToDevice);
  int rc = e == hipSuccess ? fv::launch_rope(static_cast<bf16_t*>(qkv), tab, ld, rows, T, heads, kv_heads, D, static_cast<hipStream_t>(s))
                           : fv_hip_fail(e, "hipMemcpy(rope table)");
  (void)hipStreamSynchronize(static_cast<hipStream_t>(s));
  (void)hipFree(tab);
  return rc;
}

int fv_op_attention_bwd_routes(const float* qkv, int ld, const float* dO, int lddo, float* dqkv, void* out_bf16, int ldo, float* stat, float* part, int B, int T,
                               int heads, int kv_heads, int D, const int32_t* lens, int len_add, float theta, int use_split, fv_stream st) {
  // everything is checked before the first allocation or launch: a refused call writes nothing
  if (!qkv || !dO || !dqkv || !out_bf16 || !stat) return fv_fail(FV_ERR_ARG, "attention_bwd: null pointer");
  if (D != 64 && D != 128) return fv_fail(FV_ERR_UNSUPPORTED, "attention_bwd: head_dim must be 64 or 128 (got %d)", D);
  if (B <= 0 || T <= 0 || heads <= 0 || kv_heads <= 0 || heads % kv_heads)
    return fv_fail(FV_ERR_ARG, "attention_bwd: bad shape B=%d T=%d heads=%d kv_heads=%d (heads must be a multiple of kv_heads)", B, T, heads, kv_heads);
  const int qd = heads * D;
  if (ld % 4 || ld < (heads + 2 * kv_heads) * D) return fv_fail(FV_ERR_ARG, "attention_bwd: ld = %d must be a multiple of 4 and >= (heads + 2 kv_heads) D = %d", ld, (heads + 2 * kv_heads) * D);
  if (lddo % 4 || lddo < qd) return fv_fail(FV_ERR_ARG, "attention_bwd: lddo = %d must be a multiple of 4 and >= heads D = %d", lddo, qd);
  if (ldo % 8 || ldo < 2 * qd) return fv_fail(FV_ERR_ARG, "attention_bwd: ldo = %d must be a multiple of 8 and >= 2 heads D = %d (hi | lo halves)", ldo, 2 * qd);
  hipStream_t s = static_cast<hipStream_t>(st);
  std::vector<float> cs((size_t)T * D);
  fv::rope_table_host(cs.data(), T, D, theta);
  float2* tab = nullptr;
  FV_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&tab), cs.size() * 4));
  hipError_t e = hipMemcpy(tab, cs.data(), cs.size() * 4, hipMemcpyHostToDevice);
  int rc = e == hipSuccess ? FV_OK : fv_hip_fail(e, "hipMemcpy(rope table)");
  bf16_t* o = static_cast<bf16_t*>(out_bf16);
  float* lse = stat;
  float* delta = stat + (size_t)B * heads * T;
  const float scale = 1.0f / sqrtf((float)D);
  void* scr = nullptr;   // the split-bf16 kernels' K / V records (the training path keeps this in its workspace); without it both launches take the fp32-MFMA kernels
  if (rc == FV_OK && use_split) { e = hipMalloc(&scr, fv::attention_split_scratch_bytes(B, T, kv_heads, D)); if (e != hipSuccess) rc = fv_hip_fail(e, "hipMalloc(attention scratch)"); }
  if (rc == FV_OK) rc = fv::launch_attention_f32(const_cast<float*>(qkv), ld, o, o + qd, ldo, B, T, heads, kv_heads, D, lens, len_add, scale, s, tab, nullptr, 0, 0, lse, 0, scr);
  if (rc == FV_OK) rc = fv::launch_attention_bwd(qkv, ld, o, o + qd, ldo, dO, lddo, lse, delta, dqkv, B, T, heads, kv_heads, D, lens, len_add, scale, tab, s, part, scr);
  (void)hipStreamSynchronize(s);
  (void)hipFree(tab);
  if (scr) (void)hipFree(scr);
  return rc;
}

int fv_op_attention_bwd(const float* qkv, int ld, const float* dO, float* dqkv, void* out_bf16_scratch, float* stat_scratch, int B, int T,
                        int heads, int kv_heads, int D, const int32_t* lens, float theta, fv_stream st) {
  return fv_op_attention_bwd_routes(qkv, ld, dO, heads * D, dqkv, out_bf16_scratch, 2 * heads * D, stat_scratch, nullptr, B, T, heads, kv_heads, D, lens, 0, theta, 1, st);
}

int fv_op_attention_f32(void* qkv, int ld, void* out, int ldo, int B, int T, int heads, int kv_heads, int D, const int32_t* lens, int len_add,
                        const void* rope_table, const void* pre, int ldp, int Np, float* lse, int lo8, int use_split, fv_stream st) {
  if (!qkv || !out) return fv_fail(FV_ERR_ARG, "attention_f32: null pointer");
  if (B <= 0 || T <= 0 || heads <= 0 || kv_heads <= 0 || (D != 32 && D != 64 && D != 128) || ldo < 2 * heads * D)
    return fv_fail(FV_ERR_ARG, "attention_f32: bad shape (ldo must hold the hi and lo halves)");
  hipStream_t s = static_cast<hipStream_t>(st);
  const int qd = heads * D;
  bf16_t* o = static_cast<bf16_t*>(out);
  const float scale = 1.0f / sqrtf((float)D);
  void* scr = nullptr;   // the split-bf16 kernels' K / V records, for this call only
  if (use_split) {
    if (D < 64) return fv_fail(FV_ERR_UNSUPPORTED, "attention_f32: the split-bf16 kernels need head_dim 64 / 128");
    hipError_t e = hipMalloc(&scr, fv::attention_split_scratch_bytes(B, T, kv_heads, D));
    if (e != hipSuccess) return fv_hip_fail(e, "hipMalloc(attention scratch)");
  }
  const int rc = fv::launch_attention_f32(static_cast<float*>(qkv), ld, o, o + qd, ldo, B, T, heads, kv_heads, D, lens, len_add, scale, s,
                                          static_cast<const float2*>(rope_table), static_cast<const float*>(pre), ldp, Np, lse, lo8, scr);
  if (scr) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(scr);
  }
  return rc;
}

int fv_op_rmsnorm_forms(const float* x, const float* w, void* y, void* y_lo, int ldy, int rows, int H, float eps, int f16, unsigned* sat, int lo8, fv_stream s) {
  return fv::launch_rmsnorm(x, w, static_cast<bf16_t*>(y), static_cast<bf16_t*>(y_lo), ldy, rows, H, eps, static_cast<hipStream_t>(s), f16, sat, lo8);
}

int fv_op_embed_gather(const int32_t* ids, const void* table, const float* img_tokens, float* x, int B, int T, int Ni, int H, int vocab, fv_stream s) {
  return fv::launch_embed_gather(ids, static_cast<const bf16_t*>(table), img_tokens, x, B, T, Ni, H, vocab, static_cast<hipStream_t>(s));
}

int fv_op_pool_norm(const float* x, const int32_t* lens, const float* w, float* pooled, int B, int Ttot, int Ni, int H, float eps, int mode, fv_stream s) {
  return fv::launch_pool_norm(x, lens, w, pooled, B, Ttot, Ni, H, eps, mode, static_cast<hipStream_t>(s));
}

int fv_op_rmsnorm_bwd(const float* x, const float* w, const float* dy, const float* dres, float* dx, float* dw, float* scratch, int rows,
                      int H, float eps, fv_stream s) {
  return fv::launch_rmsnorm_bwd(x, w, dy, dres, dx, dw, scratch, rows, H, eps, static_cast<hipStream_t>(s));
}

int fv_op_se_gelu(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y,
                  float* scratch, int B, int P, int C, int R, fv_stream s) {
  return fv::launch_se_gelu(static_cast<const bf16_t*>(x), w1, b1, w2, b2, static_cast<bf16_t*>(y), scratch, B, P, C, R, static_cast<hipStream_t>(s));
}

int fv_op_dwconv_mfma(const void* x, const void* ttab, const float* bias, void* y, int B, int H, int W, int C, int k, int gelu,
                      fv_stream s) {
  return fv::launch_dwconv_mfma(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(ttab), bias, static_cast<bf16_t*>(y), B, H, W, C, k,
                                gelu, static_cast<hipStream_t>(s));
}
int fv_op_dwconv_s2_mfma(const void* x, const void* ttab, const float* bias, void* y, int B, int H, int W, int C, int gelu, fv_stream s) {
  return fv::launch_dwconv_s2_mfma(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(ttab), bias, static_cast<bf16_t*>(y), B, H, W, C,
                                   gelu, static_cast<hipStream_t>(s));
}
int fv_op_dwconv_pair(const void* x, const void* t3, const float* b3, const void* t7, const float* b7, void* y1, void* y2, int B,
                      int H, int W, int C, fv_stream s) {
  return fv::launch_dwconv_pair(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(t3), b3, static_cast<const bf16_t*>(t7), b7,
                                static_cast<bf16_t*>(y1), static_cast<bf16_t*>(y2), B, H, W, C, static_cast<hipStream_t>(s));
}

int fv_op_convffn(const void* x, const void* w1, const float* b1, const void* w2p, const float* b2, const float* ls,
                  const void* res, void* out, int M, int C, fv_stream s) {
  return fv::launch_convffn(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(w1), b1, static_cast<const bf16_t*>(w2p), b2, ls,
                            static_cast<const bf16_t*>(res), static_cast<bf16_t*>(out), M, C, 4 * C, static_cast<hipStream_t>(s));
}

int fv_op_convffn32(const void* x, const void* wq, const float* b1, const float* b2, const float* ls, const void* res, void* out,
                    int M, int C, fv_stream s) {
  return fv::launch_convffn32(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(wq), b1, b2, ls, static_cast<const bf16_t*>(res),
                              static_cast<bf16_t*>(out), M, C, 4 * C, static_cast<hipStream_t>(s));
}

int fv_op_convffn32_stash(const void* x, const void* wq, const float* b1, const float* b2, const float* ls, const void* res, void* out,
                          int M, int C, void* stash_y, fv_stream s) {
  if (!stash_y) return fv_fail(FV_ERR_ARG, "fv_op_convffn32_stash: null stash");
  return fv::launch_convffn32(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(wq), b1, b2, ls, static_cast<const bf16_t*>(res),
                              static_cast<bf16_t*>(out), M, C, 4 * C, static_cast<hipStream_t>(s), nullptr, 0, static_cast<bf16_t*>(stash_y));
}
// fv_op_gemm_f16 with FV_EPI_MUL_GELUP and its second output: out f16 = acc * gelu'(4 aux), h_out f16 = gelu(4 aux) rounded to bf16
int fv_op_gemm_f16_gelup(const void* A, int lda, const void* W, int M, int N, int K, const void* aux, int ldaux, void* out, int ldo, void* h_out, fv_stream s) {
  fv::GemmArgs g{static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(W), M, N, K, nullptr, nullptr, aux, ldaux, out, ldo, FV_EPI_MUL_GELUP};
  g.f16 = 1;
  g.stash = h_out;
  return fv::launch_gemm(g, static_cast<hipStream_t>(s));
}

// tap + bias gradients of a depthwise conv (the kernels behind the tower's backward): x bf16 (B,H,W,C), dy fp16 (B,Ho,Wo,C*mult) -> dw f32 tap-major [k*k][C*mult], db [C*mult]
int fv_op_dw_wgrad(const void* x, const void* dy, float* dw, float* db, float* scratch, size_t scratch_floats, int B, int H, int W, int C, int k, int stride, int mult, fv_stream s) {
  const int pad = k / 2, Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  if (scratch_floats < fv::dw_bwd_scratch_floats(B, Ho, Wo, C * mult, k)) return fv_fail(FV_ERR_ARG, "fv_op_dw_wgrad: scratch too small (%zu floats needed)", fv::dw_bwd_scratch_floats(B, Ho, Wo, C * mult, k));
  return fv::launch_dw_wgrad(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(dy), dw, db, scratch, B, H, W, C, k, stride, mult, static_cast<hipStream_t>(s));
}

// input gradient of a depthwise / channel-multiplier conv, both routes of the tower's backward.  Every argument is checked here, before the launcher is entered:
// a refused call enqueues nothing
static bool dw_op_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int fv_op_dw_dgrad(const void* dy, const float* w, const void* res, void* dx, int B, int Hi, int Wi, int Ci, int k, int stride, int mult, int round_w, unsigned* sat,
                   fv_stream s) {
  if (!dy || !w || !dx) return fv_fail(FV_ERR_ARG, "fv_op_dw_dgrad: null pointer");
  if (!dw_op_aligned16(dy) || !dw_op_aligned16(w) || !dw_op_aligned16(res) || !dw_op_aligned16(dx) || (reinterpret_cast<uintptr_t>(sat) & 3))
    return fv_fail(FV_ERR_ARG, "fv_op_dw_dgrad: dy, w, res, dx must be 16-byte aligned");
  if (B <= 0 || Hi <= 0 || Wi <= 0 || Ci <= 0 || Ci % 8) return fv_fail(FV_ERR_ARG, "fv_op_dw_dgrad: bad shape B=%d %dx%d C=%d", B, Hi, Wi, Ci);
  const bool inst = (k == 3 && stride == 1 && mult == 1) || (k == 7 && stride == 1 && mult == 1) || (k == 3 && stride == 2 && mult == 1) ||
                    (k == 7 && stride == 2 && mult == 2) || (k == 3 && stride == 1 && mult == 2);
  if (!inst) return fv_fail(FV_ERR_UNSUPPORTED, "fv_op_dw_dgrad: unsupported k=%d stride=%d mult=%d", k, stride, mult);
  if (round_w != 0 && round_w != 1) return fv_fail(FV_ERR_ARG, "fv_op_dw_dgrad: round_w is 0 or 1");
  return fv::launch_dw_dgrad(static_cast<const bf16_t*>(dy), w, static_cast<const bf16_t*>(res), static_cast<bf16_t*>(dx), B, Hi, Wi, Ci, k, stride, mult, sat,
                             static_cast<hipStream_t>(s), round_w);
}
int fv_op_dw_dgrad_mfma(const void* dy, const void* ttab16, const void* res, void* dx, int B, int H, int W, int C, int k, unsigned* sat, fv_stream s) {
  if (!dy || !ttab16 || !dx) return fv_fail(FV_ERR_ARG, "fv_op_dw_dgrad_mfma: null pointer");
  if (!dw_op_aligned16(dy) || !dw_op_aligned16(ttab16) || !dw_op_aligned16(res) || !dw_op_aligned16(dx) || (reinterpret_cast<uintptr_t>(sat) & 3))
    return fv_fail(FV_ERR_ARG, "fv_op_dw_dgrad_mfma: dy, ttab16, res, dx must be 16-byte aligned");
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return fv_fail(FV_ERR_ARG, "fv_op_dw_dgrad_mfma: bad shape B=%d %dx%d C=%d", B, H, W, C);
  if (!fv::dw_dgrad_mfma_supported(H, W, C, k)) return fv_fail(FV_ERR_UNSUPPORTED, "fv_op_dw_dgrad_mfma: unsupported shape H=%d W=%d C=%d k=%d", H, W, C, k);
  return fv::launch_dw_dgrad_mfma(static_cast<const bf16_t*>(dy), static_cast<const bf16_t*>(ttab16), static_cast<const bf16_t*>(res), static_cast<bf16_t*>(dx), B, H,
                                  W, C, k, sat, static_cast<hipStream_t>(s));
}

int fv_op_convffn32_split(const void* x, const void* wq, const float* b1, const float* b2, const float* ls, const void* res, void* out,
                          int M, int C, float* part, size_t part_bytes, fv_stream s) {
  return fv::launch_convffn32(static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(wq), b1, b2, ls, static_cast<const bf16_t*>(res),
                              static_cast<bf16_t*>(out), M, C, 4 * C, static_cast<hipStream_t>(s), part, part_bytes);
}

// the direct LoRA backward's kernels alone (lora_direct_kernels.hip): ONE packed tensor (kind 0 plain, 1 q|k|v, 2 gate/up) with adapters on the parts in
// part_mask (bit p: part p); a_off / b_off per PART (floats into lora / lora_grads).  dY fp16 rows [R][Np]; X split bf16 (xkind 2) or fp16 (xkind 3) rows
int fv_op_lora_direct_scratch_floats(int R, int rank, int max_cols, size_t* out_floats) {
  if (!out_floats || R <= 0 || rank < 1 || rank > 64 || max_cols <= 0) return fv_fail(FV_ERR_ARG, "fv_op_lora_direct_scratch_floats: bad arguments");
  *out_floats = fv::lora_direct_scratch_floats(R, rank, max_cols);
  return FV_OK;
}
int fv_op_lora_direct(int kind, int part_mask, int rank, int Np, int K, int qd, int kd, const int64_t* a_off, const int64_t* b_off, const void* dY, const void* X,
                      int xkind, int ldx, int lo_off, int R, const float* lora, float* lora_grads, float scale, float* scratch, size_t scratch_floats, fv_stream s) {
  if (!a_off || !b_off) return fv_fail(FV_ERR_ARG, "fv_op_lora_direct: null offsets");
  const int nparts = kind == 1 ? 3 : (kind == 2 ? 2 : 1);
  if (kind < 0 || kind > 2 || part_mask <= 0 || part_mask >= (1 << nparts)) return fv_fail(FV_ERR_ARG, "fv_op_lora_direct: kind %d, part mask 0x%x", kind, part_mask);
  fv::LoraDirectPack pk{};
  pk.kind = kind; pk.r = rank; pk.Np = Np; pk.K = K; pk.qd = qd; pk.kd = kd;
  for (int p = 0; p < 3; ++p) {
    pk.slot_of_part[p] = -1;
    if (p < nparts && (part_mask >> p & 1)) { pk.slot_of_part[p] = pk.nm; pk.a_off[pk.nm] = a_off[p]; pk.b_off[pk.nm] = b_off[p]; ++pk.nm; }
  }
  pk.NCp = (pk.nm * rank + 31) / 32 * 32;
  return fv::launch_lora_direct(pk, static_cast<const bf16_t*>(dY), static_cast<const bf16_t*>(X), xkind, ldx, lo_off, R, lora, lora_grads, scale, scratch,
                                scratch_floats, static_cast<hipStream_t>(s));
}

int fv_op_chunk_loss(const float* a, const float* t, const uint8_t* pad, float* g, float* partial, size_t partial_floats, float* loss, float* metrics,
                     int64_t n, int A, int kind, float beta, float loss_scale, fv_stream s) {
  if (partial_floats < fv::chunk_loss_partial_floats()) return fv_fail(FV_ERR_ARG, "fv_op_chunk_loss: partial needs %zu floats", fv::chunk_loss_partial_floats());
  return fv::launch_chunk_loss(a, t, pad, g, partial, loss, metrics, (long)n, A, kind, beta, loss_scale, static_cast<hipStream_t>(s));
}

int fv_op_head_loss_backward(int feat, int ds, int da, int hid, int fus, int time_dim, const float* P, const float* actions, const float* targets,
                             const uint8_t* pad, int kind, float beta, int chunk, int B, const void* saved, float* loss, float* metrics, float* G,
                             float* scratch, size_t scratch_floats, float* d_pooled, fv_stream s) {
  if (feat < 1 || ds < 1 || da < 1 || hid < 1 || fus < 1 || time_dim < 0 || B < 1) return fv_fail(FV_ERR_ARG, "fv_op_head_loss_backward: bad dimensions");
  if (!metrics || !d_pooled) return fv_fail(FV_ERR_ARG, "fv_op_head_loss_backward: null pointer");
  fv::HeadDims d{feat, ds, da, hid, fus};
  d.te = time_dim;
  if (scratch_floats * sizeof(float) < fv::head_bwd_scratch_bytes(d, B))
    return fv_fail(FV_ERR_ARG, "fv_op_head_loss_backward: scratch needs %zu floats", fv::head_bwd_scratch_bytes(d, B) / sizeof(float));
  const fv::HeadLoss hl{kind, beta, chunk, pad, metrics};
  return fv::launch_head_backward(d, P, nullptr, actions, targets, B, 0.f, static_cast<const float*>(saved), loss, G, scratch, static_cast<hipStream_t>(s), d_pooled,
                                  1.0f, &hl);
}

// fv_op_head_loss_backward with `draws` noise draws per observation (fv_head_set_flow_draws): actions, targets have draws * B rows, pad (B, chunk) and d_pooled
// (B, feat) stay per observation -- d_pooled comes out summed over the draws.  dim_w (da / chunk) and step_w (chunk): device weights, both or neither
int fv_op_head_loss_backward_draws(int feat, int ds, int da, int hid, int fus, int time_dim, int draws, const float* P, const float* actions, const float* targets,
                                   const uint8_t* pad, const float* dim_w, const float* step_w, int kind, float beta, int chunk, int B, const void* saved, float* loss,
                                   float* metrics, float* G, float* scratch, size_t scratch_floats, float* d_pooled, fv_stream s) {
  if (feat < 1 || ds < 1 || da < 1 || hid < 1 || fus < 1 || time_dim < 2 || draws < 1 || draws > 16 || B < 1) return fv_fail(FV_ERR_ARG, "fv_op_head_loss_backward_draws: bad dimensions");
  if (!metrics || !d_pooled) return fv_fail(FV_ERR_ARG, "fv_op_head_loss_backward_draws: null pointer");
  fv::HeadDims d{feat, ds, da, hid, fus};
  d.te = time_dim;
  d.draws = draws;
  if (scratch_floats * sizeof(float) < fv::head_bwd_scratch_bytes(d, B))
    return fv_fail(FV_ERR_ARG, "fv_op_head_loss_backward_draws: scratch needs %zu floats", fv::head_bwd_scratch_bytes(d, B) / sizeof(float));
  if (!dim_w != !step_w) return fv_fail(FV_ERR_ARG, "fv_op_head_loss_backward_draws: give both weight vectors or neither");
  const fv::HeadLoss hl{kind, beta, chunk, pad, metrics, dim_w, step_w};
  return fv::launch_head_backward(d, P, nullptr, actions, targets, B, 0.f, static_cast<const float*>(saved), loss, G, scratch, static_cast<hipStream_t>(s), d_pooled,
                                  1.0f, &hl);
}

int fv_op_chunk_loss_weighted(const float* a, const float* t, const uint8_t* pad, const float* dim_w, const float* step_w, float* g, float* partial,
                              size_t partial_floats, float* loss, float* metrics, int64_t n, int A, int K, int kind, float beta, float loss_scale, fv_stream s) {
  if (partial_floats < fv::chunk_loss_partial_floats()) return fv_fail(FV_ERR_ARG, "fv_op_chunk_loss_weighted: partial needs %zu floats", fv::chunk_loss_partial_floats());
  if (!dim_w || !step_w) return fv_fail(FV_ERR_ARG, "fv_op_chunk_loss_weighted: null weight vector");
  return fv::launch_chunk_loss(a, t, pad, g, partial, loss, metrics, (long)n, A, kind, beta, loss_scale, static_cast<hipStream_t>(s), dim_w, step_w, K);
}

int fv_op_bins_loss(const float* logits, const float* targets, const uint8_t* pad, const float* dim_w, const float* step_w, const float* range, int n_range,
                    float sigma, int decode, float* g, float* partial, size_t partial_floats, float* loss, float* metrics, int64_t n, int bins, int da, int K,
                    float loss_scale, fv_stream s) {
  if (n < 1 || partial_floats < fv::bins_loss_partial_floats((long)n)) return fv_fail(FV_ERR_ARG, "fv_op_bins_loss: partial needs 4 * ceil(n / 4) floats");
  const fv::HeadBins hb{range, n_range, sigma, decode};
  return fv::launch_bins_loss(hb, logits, targets, pad, g, partial, loss, metrics, (long)n, bins, da, K, loss_scale, static_cast<hipStream_t>(s), dim_w, step_w);
}

int fv_op_bins_decode(const float* logits, const float* range, int n_range, int decode, float* actions, float* probs, int64_t n, int bins, int da,
                      const float* post_scale, const float* post_shift, fv_stream s) {
  const fv::HeadBins hb{range, n_range, 0.f, decode};
  return fv::launch_bins_decode(hb, logits, actions, probs, (long)n, bins, da, post_scale, post_shift, static_cast<hipStream_t>(s));
}

int fv_op_flow_vjp(int feat, int ds, int da, int hid, int fus, int time_dim, const float* freq, const float* P, const float* pooled, const float* states, int B,
                   const float* x, float t, const float* omega, float* v_out, float* jt_out, float* scratch, size_t scratch_floats, fv_stream s) {
  if (feat < 1 || ds < 1 || da < 1 || hid < 1 || fus < 1 || time_dim < 2 || time_dim % 2 || B < 1) return fv_fail(FV_ERR_ARG, "fv_op_flow_vjp: bad dimensions");
  fv::HeadDims d{feat, ds, da, hid, fus};
  d.te = time_dim;
  if (scratch_floats * sizeof(float) < fv::flow_guided_scratch_bytes(d, B))
    return fv_fail(FV_ERR_ARG, "fv_op_flow_vjp: scratch needs %zu floats", fv::flow_guided_scratch_bytes(d, B) / sizeof(float));
  return fv::launch_flow_vjp(d, fv::HeadFlow{freq, 0, 0.f, 0.f}, P, pooled, states, B, x, t, omega, v_out, jt_out, scratch, static_cast<hipStream_t>(s));
}

// fv_op_flow_vjp on a prefix-width head (fv_head_set_flow_prefix): fusion.0 has prefix_chunk more columns behind phi(t), which the chain never reads (m = 0)
int fv_op_flow_vjp_prefix(int feat, int ds, int da, int hid, int fus, int time_dim, int prefix_chunk, const float* freq, const float* P, const float* pooled,
                          const float* states, int B, const float* x, float t, const float* omega, float* v_out, float* jt_out, float* scratch, size_t scratch_floats,
                          fv_stream s) {
  if (feat < 1 || ds < 1 || da < 1 || hid < 1 || fus < 1 || time_dim < 2 || time_dim % 2 || B < 1) return fv_fail(FV_ERR_ARG, "fv_op_flow_vjp_prefix: bad dimensions");
  if (prefix_chunk < 2 || da % prefix_chunk) return fv_fail(FV_ERR_ARG, "fv_op_flow_vjp_prefix: prefix_chunk=%d must be >= 2 and divide da=%d", prefix_chunk, da);
  fv::HeadDims d{feat, ds, da, hid, fus};
  d.te = time_dim;
  d.pk = prefix_chunk;
  d.pd = 1;
  if (scratch_floats * sizeof(float) < fv::flow_guided_scratch_bytes(d, B))
    return fv_fail(FV_ERR_ARG, "fv_op_flow_vjp_prefix: scratch needs %zu floats", fv::flow_guided_scratch_bytes(d, B) / sizeof(float));
  return fv::launch_flow_vjp(d, fv::HeadFlow{freq, 0, 0.f, 0.f}, P, pooled, states, B, x, t, omega, v_out, jt_out, scratch, static_cast<hipStream_t>(s));
}

// where fusion.0's input `cat` lies inside the saved activations of a head with these dimensions (time_dim 0: the regression head; draws, prefix_chunk as
// fv_head_set_flow_draws / fv_head_set_flow_prefix set them, 1 / 0 = off): *out_floats = its offset in floats; its shape is (draws * B, cat width)
int fv_op_head_saved_cat_offset(int feat, int ds, int da, int hid, int fus, int time_dim, int draws, int prefix_chunk, int B, size_t* out_floats) {
  if (!out_floats || feat < 1 || ds < 1 || da < 1 || hid < 1 || fus < 1 || time_dim < 0 || draws < 1 || draws > 16 || prefix_chunk < 0 || B < 1)
    return fv_fail(FV_ERR_ARG, "fv_op_head_saved_cat_offset: bad arguments");
  fv::HeadDims d{feat, ds, da, hid, fus};
  d.te = time_dim;
  d.draws = draws;
  d.pk = time_dim > 0 ? prefix_chunk : 0;
  *out_floats = fv::head_saved_cat_offset(d, B);
  return FV_OK;
}

int fv_op_flow_select(const float* cand, int B, int S, int da, int select, const float* prev, int shift, const int32_t* row_mask, const float* step_w, int chunk,
                      const float* post_scale, const float* post_shift, float* actions, float* chunk_out, float* candidates_out, int32_t* choice_out,
                      float* scores_out, float* spread_out, fv_stream s) {
  const fv::FlowSelect sel{select, prev, shift, row_mask, step_w, chunk, actions, chunk_out, candidates_out, choice_out, scores_out, spread_out};
  return fv::launch_flow_select(cand, B, S, da, sel, post_scale, post_shift, static_cast<hipStream_t>(s));
}

}  // extern "C"

// the step guard's saturation flag, set as a run of saturating casts would leave it (fv_step_guard_flag hands out the address): one float, stream-ordered
namespace {
__global__ void set_float_kernel(float* dst, float value) { *dst = value; }
}  // namespace
extern "C" int fv_op_step_guard_set_flag(float* flag_dev, float value, fv_stream s) {
  if (!flag_dev || !(value >= 0.f)) return fv_fail(FV_ERR_ARG, "fv_op_step_guard_set_flag: a flag address and a value >= 0");
  hipLaunchKernelGGL(set_float_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(s), flag_dev, value);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
