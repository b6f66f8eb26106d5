/* fastvla_hip_testops.h -- TEST-ONLY op-level entry points (one kernel each) over the internals of libfastvla_hip.so.
 *
 * Built by `make -C vla-from-fastvlm_amd/csrc` into vla-from-fastvlm_amd/testops/libfastvla_hip_testops.so (csrc/ops_api.hip); its undefined `fv::launch_*`
 * references resolve against an already loaded libfastvla_hip.so (fastvla_hip._lib.load_testops() loads the product library RTLD_GLOBAL first).
 * Nothing of the product (fastvla_hip/, vla_fastvlm/, bench.py's timed region, __graft_entry__) binds these symbols: they exist so that
 * tests/test_gpu_ops.py, its sibling op-level files (tests/test_gpu_dw_backward.py: every kernel instance and route of the depthwise backward, input gradient
 * included) and tools/ can check and time each kernel on its own against the oracle's op.  The product ABI a maintainer binds is
 * include/fastvla_hip.h alone.  (The epilogue enum lives here because only these entry points take it as an argument; the library's own
 * sources include this header for it.) */
#ifndef FASTVLA_HIP_TESTOPS_H
#define FASTVLA_HIP_TESTOPS_H

#include "fastvla_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- op-level entry points (used by the parity tests to check each kernel on its own) ------------------------- */
enum fv_gemm_epilogue {
  FV_EPI_BIAS = 0,        /* out bf16 = acc + bias                                  */
  FV_EPI_BIAS_GELU = 1,   /* out bf16 = gelu(acc + bias)                            */
  FV_EPI_LS_RES = 2,      /* out bf16 = res_bf16 + scale[n] * (acc + bias[n])       */
  FV_EPI_RES_F32 = 3,     /* out f32  = res_f32 + acc (+ bias)                      */
  FV_EPI_SWIGLU = 4,      /* out bf16[M,N/2] = silu(gate) * up, W rows 8-interleaved */
  FV_EPI_F32 = 5,         /* out f32  = acc + bias                                  */
  FV_EPI_SWIGLU_SPLIT = 7,/* out bf16[M,N] = [hi | lo] of silu(gate)*up (split-bf16 operand), W rows 8-interleaved */
  FV_EPI_SWIGLU_F16 = 8,  /* out f16[M,N/2] = silu(gate)*up / 16 (the fp16 operand of the down projection, whose fp16 weights carry the
                           * 16: the power of two keeps SwiGLU outputs up to 1e6 inside fp16's range), W rows 8-interleaved */
  /* the tower backward's three (all 2-byte outputs are fp16, saturating, whatever the operand type) */
  FV_EPI_GELU_GRAD = 9,   /* a = acc + bias: out f16 = gelu(a) (the 5e-5 minimax Phi of the forward kernels, rounded to a bf16 value first; out may be NULL), stash f16 = gelu'(a), both [M][ldo] */
  FV_EPI_MUL_AUX = 10,    /* out f16 = acc * aux_f16[m][n] (aux = res, row stride ldr; out may alias aux)                              */
  FV_EPI_F16 = 11,        /* out f16 = acc + bias                                                                                      */
  FV_EPI_MUL_GELUP = 12   /* out f16 = acc * gelu'(4 * aux_f16[m][n]); stash f16 (optional) = gelu(4 * aux) rounded to bf16: aux = the pre-activation / 4 the training forward's fused ConvFFN stashed (round 6) */
};
/* out[M,N] = A[M,K] (bf16, row stride lda) x W[N,K]^T (bf16) with fp32 accumulation on MFMA */
int fv_op_gemm(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const float* scale,
               const void* res, int ldr, void* out, int ldo, int epilogue, fv_stream s);
/* the split-bf16 form the parity-mode decoder uses: A (M, 2K) carries [hi | lo] halves side by side (lda >= 2K), and
 * out = (A_hi + A_lo) . W^T in one launch with a doubled K loop; epilogues as fv_op_gemm */
/* fp16 operands (A and W hold IEEE binary16 bits), fp32 accumulation on v_mfma_f32_16x16x32_f16; epilogues as fv_op_gemm plus
 * FV_EPI_SWIGLU_F16 (the path of llm_precision = 2's gate/up and down projections) */
int fv_op_gemm_f16(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const void* res, int ldr, void* out,
                   int ldo, int epilogue, void* ws, size_t ws_bytes, fv_stream s);
/* the "hi + lo8" form of llm_precision = 5: A rows = K bf16 values, then at byte offset 2K their K remainders as fp8 e4m3 (x 2^8); W8 = fp8 copy
 * of W x 2^6 at row stride 2K bytes.  out = (A_hi + A_lo8 2^-8) . W^T with the lo product on v_mfma_scale_f32_16x16x128_f8f6f4 against W8: 1.5
 * passes.  K % 128 == 0, lda >= 1.5 K.  fv_op_lo8_pack builds both operand forms from fp32 rows / a bf16 weight (either may be NULL). */
int fv_op_gemm_lo8(const void* A, int lda, const void* W, const void* W8, int M, int N, int K, const float* bias, const void* res, int ldr, void* out,
                   int ldo, int epilogue, void* ws, size_t ws_bytes, fv_stream s);
int fv_op_lo8_pack(const float* x, void* a_out, int lda, const void* W, void* w8_out, int M, int K, int N, fv_stream s);
int fv_op_gemm_ksplit(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const void* res, int ldr,
                      void* out, int ldo, int epilogue, fv_stream s);
/* fv_op_gemm_ksplit (ksplit != 0) or fv_op_gemm with a caller-owned scratch buffer for split-K partial sums: fp32 epilogues
 * (FV_EPI_RES_F32 / FV_EPI_F32) of problems with few output tiles and a long K are cut along K, one unit per CU, and
 * summed by a second kernel.  ws may be NULL (then exactly fv_op_gemm / fv_op_gemm_ksplit). */
/* out f32[M,N] = sum_k A[k][m] W[k][n] (+ bias[n]): both operands row-major over the CONTRACTION index (A [K][M] row stride lda, W [K][N] row stride
 * ldw; bf16, or fp16 bits with f16 != 0), K % 64 == 0, M % 8 == 0, N % 8 == 0 -- the weight-gradient shape (fv_train_set_options wgrad_f16 = 2) */
int fv_op_gemm_tn(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int f16, const float* bias, void* out, int ldo, void* ws,
                  size_t ws_bytes, fv_stream s);
int fv_op_gemm_splitk(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const void* res, int ldr,
                      void* out, int ldo, int epilogue, int ksplit, void* ws, size_t ws_bytes, fv_stream s);
/* fv_op_gemm_splitk with the decoder's remaining launch settings: scale[N] (FV_EPI_LS_RES, also behind K ranges), few_rows (0 = never the few-row K-range
 * forms: the training path) and an RMSNorm of the fp32 output rows (norm_w[N] non-NULL; fp32 epilogues, ldo == N): norm_y (+ norm_ylo, may be NULL) = bf16
 * hi (+ lo) of norm_w * out * rsqrt(mean(out^2) + norm_eps), row stride norm_ld -- fused into the split-K reducer where K ranges are taken, a separate
 * launch otherwise */
int fv_op_gemm_norm(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const float* scale, const void* res, int ldr, void* out,
                    int ldo, int epilogue, int ksplit, void* ws, size_t ws_bytes, int few_rows, const float* norm_w, void* norm_y, void* norm_ylo, int norm_ld,
                    float norm_eps, fv_stream s);
/* What launch_gemm would do with a problem on a device of `cus` compute units, without launching anything (the library's plan_gemm: it reads no memory, so the
 * operands are given as presence flags; ws_bytes = the split-K scratch, 0: none; ksplit 0 / 1 / 2 = one operand, [hi | lo], hi + lo8).  Writes one launch to
 * out[0], or two where the tail is cut off (columns [c0, c1) each), and returns their number -- or the refusal's code (negative), with out untouched.  The names
 * are those of tests/gemm_util.py: "gemm256_kernel<8,4,ASYM>", "splitk_reduce_kernel" ("" = one pass). */
typedef struct fv_gemm_plan_launch {
  char kernel[40], reducer[40];
  int tile, tiles_m, group_m, splits, npad, grid;
  int norm;    /* the RMSNorm that follows: 0 not asked, 1 fused into the reducer, 2 a launch of its own */
  int c0, c1;
} fv_gemm_plan_launch;
int fv_op_gemm_plan(int M, int N, int K, int lda, int ldw, int ldo, int ldr, int epilogue, int ksplit, int f16, int tn, int few_rows, int cus, size_t ws_bytes,
                    int has_bias, int has_scale, int has_res, int has_stash, int has_norm, int has_w8, fv_gemm_plan_launch* out);
/* depthwise / channel-multiplier grouped conv, NHWC bf16: x (B,H,W,C) -> y (B,Ho,Wo,C*mult); w f32 [k*k][C*mult] */
int fv_op_dwconv(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int C, int k,
                 int stride, int mult, int gelu, fv_stream s);
/* dense 3x3 stride-2 stem conv on (B,S,S,4) bf16 -> (B,S/2,S/2,Cout) bf16, + bias + GELU; w f32 [27][Cout] */
int fv_op_stem_conv(const void* pix, const float* w, const float* bias, void* y, int B, int S, int Cout, fv_stream s);
/* the same stem as an implicit GEMM on MFMA: wp (Cout,64) bf16 with slot 32*ks + 8*g + e = weight of kernel row
 * ky = 2*ks + (g>>1), column kx = 2*(g&1) + (e>>2), channel e&3 (0 where ky, kx or channel is 3); Cout % 16 == 0 */
int fv_op_stem_mfma(const void* pix, const void* wp, const float* bias, void* y, int B, int S, int Cout, fv_stream s);
/* the first two stem convolutions fused (conv 3x3 s2 3->96 + GELU, depthwise 3x3 s2 + GELU): pix (B,S,S,4) bf16 ->
 * y (B,S/4,S/4,96) bf16; wp as for fv_op_stem_mfma, w2 f32 [9][96] tap-major, the half-resolution map stays in LDS
 * (rounded to bf16 there exactly as the unfused pair rounds it to memory).  Cout must be 96, S % 4 == 0. */
int fv_op_stem_fused(const void* pix, const void* wp, const float* b1, const float* w2, const float* b2, void* y, int B,
                     int S, int Cout, fv_stream s);
/* fv_op_stem_fused reading the SOURCE images (B,C,Hin,Win) f32 | u8 through the letterbox arithmetic of fv_preprocess (the kernel behind
 * fv_vision_forward_images): y must equal fv_op_stem_fused on fv_preprocess's output bit for bit */
int fv_op_stem_fused_images(const void* img, int dtype, int B, int C, int Hin, int Win, float pad_value, int resize_with_padding, const void* wp,
                            const float* b1, const float* w2, const float* b2, void* y, int S, int Cout, fv_stream s);
/* per-pixel LayerNorm over channels (LayerNormChannel), x,y (rows,C) bf16 */
int fv_op_layernorm_rows(const void* x, const float* w, const float* b, void* y, int rows, int C, float eps,
                         fv_stream s);
/* multi-head attention on packed projections: q/k/v element pointers with row strides, heads of width D.
 * causal != 0: key j visible to query i iff j <= i; lens (B) int32 or NULL masks keys >= len. */
int fv_op_attention(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, void* out, int ldo, int B,
                    int T, int heads, int kv_heads, int D, int causal, const int32_t* lens, float scale, fv_stream s);
/* fv::launch_attention with every argument it has (fv_op_attention passes len_add = 0): key j visible to query i iff (causal == 0 or j <= i) and
 * j < clamp(lens[b] + len_add, 1, T) (lens NULL: T) -- the decoder's call has lens = text lengths and len_add = the image tokens.  q, k, v: bf16, 16-byte aligned,
 * row strides multiples of 8 and >= heads D / kv_heads D; out: bf16, 8-byte aligned, ldo % 4 == 0 and >= heads D; D in {32, 64, 128}; heads % kv_heads == 0.
 * D = 32 without masks and T % 64 == 0 runs attention32_kernel, everything else attention_kernel<D, masked>.  Rows >= the key length of q, k, v must hold FINITE
 * values (masked keys enter the P.V product with P = 0).  A refused call enqueues nothing. */
int fv_op_attention_bf16(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, void* out, int ldo, int B, int T, int heads, int kv_heads, int D,
                         int causal, const int32_t* lens, int len_add, float scale, fv_stream s);
/* the tower's attention backward alone (fv::launch_tower_attn_bwd: tattn_dq_kernel, tattn_dkv_kernel; non-causal, head_dim 32, any T): qkv bf16 rows [q | k | v], each
 * C = heads * 32 wide (row stride ld >= 3 C), dO fp16 bits (row stride lddo >= C) -> dqkv fp16 bits in qkv's column order (row stride ldd >= 3 C); stats: 2 * B * heads * T
 * floats, lse2 [B][heads][T] (log2 of the row sums of 2^(scale log2e s)) then delta [B][heads][T] (sum_j P_ij dP_ij).  Strides multiples of 8, pointers 16-byte aligned.
 * A refused call enqueues nothing. */
int fv_op_tower_attention_bwd(const void* qkv, int ld, const void* dO, int lddo, void* dqkv, int ldd, float* stats, int B, int T, int heads, float scale, fv_stream s);
int fv_op_rmsnorm(const float* x, const float* w, void* y_bf16, int rows, int H, float eps, fv_stream s);
/* in-place rotate-half RoPE on the q and k parts of a packed qkv (rows = B*T, position = row % T) */
int fv_op_rope(void* qkv, int ld, int rows, int T, int heads, int kv_heads, int D, float theta, fv_stream s);
/* backward of fv_op_attention's causal GQA form in fp32 (the kernels behind fv_train_forward_backward): qkv fp32 [B*T][ld] = UN-rotated
 * q | k | v (the rotate-half RoPE of `theta` is applied inside, as in the parity-mode forward), dO fp32 [B*T][heads*D] -> dqkv fp32 [B*T][ld]
 * (gradients w.r.t. the un-rotated projections).  Runs the forward first (its output and row statistics are scratch).  D in {64, 128}. */
int fv_op_attention_bwd(const float* qkv, int ld, const float* dO, float* dqkv, void* out_bf16_scratch, float* stat_scratch, int B, int T,
                        int heads, int kv_heads, int D, const int32_t* lens, float theta, fv_stream s);
/* fv_op_attention_bwd with every argument of fv::launch_attention_bwd the engine uses, so that each of its routes runs on its own: dO rows of stride lddo >= heads * D;
 * out_bf16: the forward's output, bf16 rows of stride ldo >= 2 * heads * D (hi halves at column 0, remainders at column heads * D); stat: lse | delta, 2 * B * heads * T
 * floats; key j visible to query i iff j <= i and j < clamp(lens[b] + len_add, 1, T).  part: NULL (dK / dV looped over the group's q heads in one block), or
 * >= (heads / kv_heads) * B * T * 2 * kv_heads * D floats: with more than one q head per kv head every q head's share of dK | dV goes to part[hh][B * T][2 * kv_heads * D]
 * and the k | v columns of dqkv are their fp32 sum in the order hh = 0, 1, ... (attn_dkv_reduce_kernel); ignored when heads == kv_heads.  use_split != 0 allocates the
 * split-bf16 kernels' scratch for the call (forward and backward then take them); 0 runs the fp32-MFMA forward and attn_bwd_dq_kernel / attn_bwd_dkv_kernel.
 * Arguments are checked before anything is enqueued (null pointers, D in {64, 128}, heads % kv_heads, ld % 4, lddo % 4, ldo % 8, the minimum widths). */
int fv_op_attention_bwd_routes(const float* qkv, int ld, const float* dO, int lddo, float* dqkv, void* out_bf16, int ldo, float* stat, float* part, int B, int T,
                               int heads, int kv_heads, int D, const int32_t* lens, int len_add, float theta, int use_split, fv_stream s);
/* the parity-mode decoder's fp32 forward attention as the engine launches it (fv::launch_attention_f32): causal GQA over qkv fp32 rows [q | k | v] (row stride ld),
 * scale = 1 / sqrt(D), key j visible to query i iff j <= i and j < clamp(lens[b] + len_add, 1, T) (lens NULL: T).  out: bf16 rows of stride ldo >= 2 * heads * D, the hi
 * halves at column 0 and the remainders at column heads * D -- bf16, or with lo8 != 0 one fp8 e4m3 byte each (x 2^8) from the lo half's byte offset on.
 * rope_table: device [T][D/2] (cos, sin) pairs the caller supplies, or NULL (qkv is then taken as already rotated).  lse: optional [B][heads][T] max + log(sum).
 * Routes: use_split != 0 allocates the split-bf16 kernels' scratch for the call (freed after a stream sync), and launch_attention_f32 then takes them when lse is
 * wanted or T >= 128 (head_dim 64 / 128, no pre, no lo8); otherwise head_dim 64 / 128 run the fp32-MFMA kernel and head_dim 32 the VALU kernel.
 * pre != NULL (head_dim 64 / 128): rows (b * Np + pos) of [k | v] fp32, un-rotated, row stride ldp, for the positions < Np; qkv and out then hold ONLY the T - Np
 * new rows of each batch entry (row b * (T - Np) + t - Np), while T, lens + len_add and the table's positions count the whole sequence.
 * The head_dim-32 route ROTATES qkv IN PLACE (its q and k parts) when a table is given; head_dim 64 / 128 leave qkv untouched. */
int fv_op_attention_f32(void* qkv, int ld, void* out, int ldo, int B, int T, int heads, int kv_heads, int D, const int32_t* lens, int len_add,
                        const void* rope_table, const void* pre, int ldp, int Np, float* lse, int lo8, int use_split, fv_stream s);
/* every output form of the decoder's RMSNorm (fv::launch_rmsnorm): y bf16 rows of stride ldy; y_lo (optional) the bf16 remainders at the same stride, or with
 * lo8 != 0 one fp8 e4m3 byte each (x 2^8) from y_lo's row starts on; f16 != 0: y receives fp16 bits, saturating at +-65504 (y_lo must be NULL), and *sat (device,
 * optional) grows by one per 8-element group that holds a clamped value */
int fv_op_rmsnorm_forms(const float* x, const float* w, void* y, void* y_lo, int ldy, int rows, int H, float eps, int f16, unsigned* sat, int lo8, fv_stream s);
/* x f32 [B][Ni + T][H]: rows t < Ni = img_tokens f32 [B][Ni][H], the others = table bf16 [vocab][H] at ids int32 [B][T] clamped to [0, vocab - 1] */
int fv_op_embed_gather(const int32_t* ids, const void* table, const float* img_tokens, float* x, int B, int T, int Ni, int H, int vocab, fv_stream s);
/* pooled f32 [B][H] from x f32 [B][Ttot][H]: mode 0 = RMSNorm of row Ni + max(len - 1, 0), mode 1 = mean of the RMSNorms of rows 0 .. Ni + len - 1;
 * len = clamp(lens[b], 0, Ttot - Ni) (lens NULL: Ttot - Ni) */
int fv_op_pool_norm(const float* x, const int32_t* lens, const float* w, float* pooled, int B, int Ttot, int Ni, int H, float eps, int mode, fv_stream s);
/* backward of fv_op_rmsnorm: y = w x rsqrt(mean(x^2) + eps); dx (rows,H) f32 = dres (or 0) + dL/dx, dw (H) f32; scratch floats:
 * ((rows + 15) / 16 + 3) / 4 * 4 * H + 64 * H */
int fv_op_rmsnorm_bwd(const float* x, const float* w, const float* dy, const float* dres, float* dx, float* dw, float* scratch, int rows,
                      int H, float eps, fv_stream s);

/* SE + GELU tail of conv_exp: x (B,P,C) bf16 -> y = gelu(x * sigmoid(W2 relu(W1 mean_p(x) + b1) + b2)) */
int fv_op_se_gelu(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y,
                  float* scratch, int B, int P, int C, int R, fv_stream s);

/* stride-1 depthwise k x k (k in {3,7}) on the matrix cores (v_mfma_f32_4x4x4_16b_bf16, one 4x4 block per channel);
 * W >= 32, C % 32 == 0.  ttab = bf16 Toeplitz table [C/16][k][NM=(k+6)/4][16 ch][4 i][4 kk] = w[ky][4m + kk - i] (0 outside
 * the kernel), i.e. the depthwise weights rounded to bf16. */
int fv_op_dwconv_mfma(const void* x, const void* ttab, const float* bias, void* y, int B, int H, int W, int C, int k, int gelu,
                      fv_stream s);
/* the PatchEmbed large-kernel conv on the same scheme: 7x7, stride 2, two output channels per input channel (groups = C):
 * x (B,H,W,C) -> y (B,H/2,W/2,2C) bf16 NHWC; H, W even, W >= 16, C % 32 == 0.  ttab = bf16 Toeplitz table
 * [C/16][e=2][7][4][16 ch][4 i][4 kk] = w[ky][4m + kk - 2i] of output channel 2 (16 g + ch) + e (0 outside the 7 taps).
 * Replaces fv_op_dwconv(k=7, stride=2, mult=2) for these shapes (mci.py PatchEmbed, lkb_reparam). */
int fv_op_dwconv_s2_mfma(const void* x, const void* ttab, const float* bias, void* y, int B, int H, int W, int C, int gelu,
                         fv_stream s);
/* RepMixer pair in one marching kernel: y1 = dw3x3(x) + b3 (the reparameterised token mixer), y2 = dw7x7(y1) + b7 (the
 * ConvFFN's conv); x, y1, y2 (B,H,W,C) bf16 NHWC, distinct; t3 / t7 Toeplitz tables as for fv_op_dwconv_mfma (k = 3 / 7);
 * H >= 16, W >= 32, C % 32 == 0. */
int fv_op_dwconv_pair(const void* x, const void* t3, const float* b3, const void* t7, const float* b7, void* y1, void* y2, int B,
                      int H, int W, int C, fv_stream s);
/* fused ConvFFN pointwise half: out (M,C) bf16 = res + ls * (fc2(gelu(fc1(x) + b1)) + b2), hidden = 4C never leaves the
 * chip.  w1 (4C,C) bf16; w2p = fc2 weight (C,4C) re-laid as [4C/32][C][32] with slot 8g+j of each 32-block holding
 * hidden 16*(j>>2) + 4*g + (j&3).  C in {32,64,96,128,192,384}.  out may alias res, not x. */
int fv_op_convffn(const void* x, const void* w1, const float* b1, const void* w2p, const float* b2, const float* ls,
                  const void* res, void* out, int M, int C, fv_stream s);

/* the same fused ConvFFN on v_mfma_f32_32x32x16_bf16 (the kernel the engine uses for C in {96,192,384}).  wq = fc1 (4C,C) / 4 and
 * 4 * fc2 (C,4C) (powers of two: exact; the kernel's GELU runs in y = x / 4 and takes b1 / 4 itself from the plain b1 it is given) as
 * ONE bf16 stream [4C/32 chunks][64 C]: per 32-hidden chunk the kernel's LDS slot image in staging order.
 * Slot image T: W1 part = 32 rows x C, 8-element chunk c of row r at chunk c ^ ((r >> SH) & MASK) with (SH, MASK) = (0,15) / (1,7) /
 * (2,3) for C = 384 / 192 / 96; W2 part = C rows x 32, chunk (2s + h) ^ ((n >> 2) & 3) of row n holding hidden
 * 16s + 8(j>>2) + 4h + (j&3), j < 8 (the k order in which a 32x32 accumulator tile, converted pairwise to bf16, is the B operand
 * of the next product).  Every KB of T is stored transposed for the add-tid LDS stores: G[8l + 2d + b] = T[128d + 2l + b],
 * l < 64, d < 4, b < 2. */
int fv_op_convffn32(const void* x, const void* wq, const float* b1, const float* b2, const float* ls, const void* res, void* out,
                    int M, int C, fv_stream s);
/* The same operator when a launch has few row tiles (one to four observations: <= 128 tiles for 256 CUs): blocks = (row tile, one of 2 / 4 / 8 ranges
 * of the hidden units), fp32 partial sums in `part` (>= ranges x M x C floats, 16-byte aligned), then one pass adds the ranges in order and applies
 * b2, ls and the residual exactly as the one-launch epilogue does.  Falls back to fv_op_convffn32 when M is large or `part` too small.  The engine
 * takes this form by itself below 128 row tiles (fv_vision_forward at B <= 4). */
/* the TRAINING forward's form of fv_op_convffn32 (round 6): the same output bits, and the pre-activation on the way out -- stash_y (M,4C) fp16 = (fc1(x) + b1) / 4
 * (round towards zero), in natural column order.  M * 8C < 2 GiB. */
int fv_op_convffn32_stash(const void* x, const void* wq, const float* b1, const float* b2, const float* ls, const void* res, void* out,
                          int M, int C, void* stash_y, fv_stream s);
/* the fc2 input gradient of the tower's backward as it runs there: fp16 operands, out f16 = (A . W^T) * gelu'(4 aux), h_out f16 (may be NULL) = gelu(4 aux) rounded to
 * a bf16 value (the fc2 weight gradient's operand), aux = fv_op_convffn32_stash's stash_y */
int fv_op_gemm_f16_gelup(const void* A, int lda, const void* W, int M, int N, int K, const void* aux, int ldaux, void* out, int ldo, void* h_out, fv_stream s);
/* tap + bias gradients of a depthwise / channel-multiplier conv as the tower's backward computes them: x bf16 (B,H,W,C), dy fp16 bits (B,Ho,Wo,C*mult) ->
 * dw f32 tap-major [k*k][C*mult], db f32 [C*mult]; scratch_floats >= (B * ceil(W / 32) or 512) * (k*k + 1) * C*mult (the call checks).  Stride-1 maps with C % 32 == 0,
 * W >= 32, H >= 16 and k = 7 run on the matrix cores (dw_wgrad_mfma_kernel, round 6), everything else on the VALU forms. */
int fv_op_dw_wgrad(const void* x, const void* dy, float* dw, float* db, float* scratch, size_t scratch_floats, int B, int H, int W, int C, int k, int stride, int mult, fv_stream s);
/* the INPUT gradient of the same convs, one entry point per route of the tower's backward (tests/test_gpu_dw_backward.py drives every kernel instance of the
 * depthwise backward through these two and fv_op_dw_wgrad): dy fp16 bits (B,Ho,Wo,Ci*mult), res (may be NULL) and dx fp16 bits (B,Hi,Wi,Ci), dx = res + conv^T(dy),
 * saturating; *sat (may be NULL) goes up by one for every (pixel, 8-channel group) cell that holds a clamped value.  Arguments are checked before anything is
 * enqueued.
 *   fv_op_dw_dgrad: dw_dgrad_kernel<k, stride, mult>, (k, stride, mult) one of (3,1,1) (7,1,1) (3,2,1) (7,2,2) (3,1,2); w fp32 tap-major [k*k][Ci*mult]; round_w = 1
 *     rounds the taps to bf16 first (the forward ran on a bf16 Toeplitz table).  A cell counts when res + conv^T(dy), summed in fp32, leaves +-65504.
 *   fv_op_dw_dgrad_mfma: dwconv_march_kernel<k, GRAD> (stride 1, mult 1, k = 3 / 7, C % 32 == 0, W >= 16, H >= 16: anything else is refused); ttab16 = the fp16
 *     Toeplitz table of the FLIPPED taps (tap t takes tap k*k-1-t).  conv^T(dy) crosses LDS in fp16 cells (two per value under a residual, so the sum is rounded
 *     once); a cell counts when conv^T(dy) itself or the final sum leaves +-65504, and a conv^T(dy) that does is written as +-65504 whatever res holds. */
int fv_op_dw_dgrad(const void* dy, const float* w, const void* res, void* dx, int B, int Hi, int Wi, int Ci, int k, int stride, int mult, int round_w, unsigned* sat,
                   fv_stream s);
int fv_op_dw_dgrad_mfma(const void* dy, const void* ttab16, const void* res, void* dx, int B, int H, int W, int C, int k, unsigned* sat, fv_stream s);
int fv_op_convffn32_split(const void* x, const void* wq, const float* b1, const float* b2, const float* ls, const void* res, void* out,
                          int M, int C, float* part, size_t part_bytes, fv_stream s);

/* the direct LoRA backward's kernels alone (csrc/lora_direct_kernels.hip), ONE packed tensor with the adapters inside it: kind 0 plain, 1 q|k|v (qd / kd wide column
 * ranges of dY), 2 gate / up interleaved by 8; part_mask bit p = part p (q / gate / the matrix, k / up, v) has an adapter; a_off / b_off[3] per PART: lora_A (rank x K) /
 * lora_B (out x rank) as float offsets into lora (parameters) and lora_grads (outputs: scale * dA, scale * dB).  dY fp16 rows [R][Np]; X [R] rows of K columns, row stride
 * ldx: xkind 2 = split bf16 (value = X[c] + X[lo_off + c]), 3 = fp16.  scratch: the float count fv_op_lora_direct_scratch_floats(R, rank, max(Np, K)) returns. */
int fv_op_lora_direct_scratch_floats(int R, int rank, int max_cols, size_t* out_floats);
int fv_op_lora_direct(int kind, int part_mask, int rank, int Np, int K, int qd, int kd, const int64_t* a_off, const int64_t* b_off, const void* dY, const void* X,
                      int xkind, int ldx, int lo_off, int R, const float* lora, float* lora_grads, float scale, float* scratch, size_t scratch_floats, fv_stream s);


/* the chunked action loss alone (csrc/chunk_kernels.hip chunk_loss_kernel + its fold; fv_head_set_loss in fastvla_hip.h has the definitions): a, t (n) f32 =
 * (B, K, A) row-major with A the step width, pad (n / A) bytes or NULL -> g (n) = loss_scale * w * rho'(a - t) / n, loss (1), metrics (2) = { masked MSE, valid
 * fraction }.  partial: scratch of partial_floats >= 768 floats.  kind FV_LOSS_*. */
int fv_op_chunk_loss(const float* a, const float* t, const uint8_t* pad, float* g, float* partial, size_t partial_floats, float* loss, float* metrics,
                     int64_t n, int A, int kind, float beta, float loss_scale, fv_stream s);

/* the same with the weights of fv_head_set_loss_weights: dim_w (A) and step_w (K) DEVICE floats, both required; (n / A) % K == 0.  om = dim_w[a] * step_w[k]
 * scales rho and g, an element with om == 0 is selected away like a padded one; the metrics stay unweighted. */
int fv_op_chunk_loss_weighted(const float* a, const float* t, const uint8_t* pad, const float* dim_w, const float* step_w, float* g, float* partial,
                              size_t partial_floats, float* loss, float* metrics, int64_t n, int A, int K, int kind, float beta, float loss_scale, fv_stream s);

/* the binned head's loss alone (csrc/bins_kernels.hip bins_loss_kernel + fold; fastvla_hip.h "binned action head" has the formulas): logits, g (n, bins)
 * DEVICE f32 with n = rows * da groups, targets (n), pad (n / (da / K)) bytes or NULL, dim_w (da / K) and step_w (K) DEVICE floats, both or neither;
 * range: DEVICE [lo | hi | w], n_range floats each (w = the fp32 (hi - lo) / bins), element e of a row reads entry e % n_range.  partial: 4 * ceil(n / 4) floats
 * of scratch; loss 1 float; metrics 4 floats. */
int fv_op_bins_loss(const float* logits, const float* targets, const uint8_t* pad, const float* dim_w, const float* step_w, const float* range, int n_range,
                    float sigma, int decode, float* g, float* partial, size_t partial_floats, float* loss, float* metrics, int64_t n, int bins, int da, int K,
                    float loss_scale, fv_stream s);
/* the decode alone (bins_decode_kernel): logits (n, bins) -> actions (n), then actions * post_scale[e] + post_shift[e] (da DEVICE floats each, both or NULL);
 * probs (n, bins) or NULL: softmax(logits) as well. */
int fv_op_bins_decode(const float* logits, const float* range, int n_range, int decode, float* actions, float* probs, int64_t n, int bins, int da,
                      const float* post_scale, const float* post_shift, fv_stream s);

/* the head's fused loss + backward (csrc/head_kernels.hip launch_head_backward) on explicit head dimensions, WITH d_pooled (B, feat): dL/d(pooled feature),
 * the gradient an unfrozen backbone continues from, which no product entry point hands out at the head level.  time_dim = E > 0: the flow head, whose cat row
 * is feat + hid + da + E wide (d_pooled is still its first feat columns).  P / G: the flat parameter / gradient buffers of that layout; actions, targets
 * (B, da); pad (B, chunk) bytes or NULL; kind FV_LOSS_*; saved: what fv_head_forward left; metrics: 4 floats; scratch: scratch_floats floats, at least
 * B * da + 2 * B * max(cat width, fus) + 64 + 768. */
int fv_op_head_loss_backward(int feat, int ds, int da, int hid, int fus, int time_dim, const float* P, const float* actions, const float* targets,
                             const uint8_t* pad, int kind, float beta, int chunk, int B, const void* saved, float* loss, float* metrics, float* G,
                             float* scratch, size_t scratch_floats, float* d_pooled, fv_stream s);
/* the same with `draws` = S noise draws per observation (fv_head_set_flow_draws; flow head only, 1 <= S <= 16): actions, targets (S B, da), draw-major; pad
 * (B, chunk) and d_pooled (B, feat) stay per observation, d_pooled summed over the draws in ascending s; saved: what fv_head_forward left on a handle with the
 * same setting.  dim_w (da / chunk) / step_w (chunk): the loss weights as device floats, both or both NULL.  scratch: with R = S B, at least
 * R * da + 2 * R * max(cat width, fus) + 64 + 768 floats, and (R * da + 3) / 4 more when S > 1. */
int fv_op_head_loss_backward_draws(int feat, int ds, int da, int hid, int fus, int time_dim, int draws, const float* P, const float* actions, const float* targets,
                                   const uint8_t* pad, const float* dim_w, const float* step_w, int kind, float beta, int chunk, int B, const void* saved, float* loss,
                                   float* metrics, float* G, float* scratch, size_t scratch_floats, float* d_pooled, fv_stream s);

/* one guided sampler step's chain alone (csrc/flow_kernels.hip launch_flow_vjp; fv_head_flow_sample_guided in fastvla_hip.h has the definitions): the
 * conditioning, the velocity v(x, t) through the step's forward kernels and J^T omega, J = dv / dx, through its three transposed products and the LayerNorm
 * backward.  Explicit head dimensions (time_dim = E > 0), freq: E / 2 DEVICE floats 2 pi / p_j; P: the flat parameters of that layout; x, omega (B, da);
 * v_out, jt_out (B, da).  scratch: scratch_floats floats; FV_ERR_ARG names the count when it is too small. */
int fv_op_flow_vjp(int feat, int ds, int da, int hid, int fus, int time_dim, const float* freq, const float* P, const float* pooled, const float* states, int B,
                   const float* x, float t, const float* omega, float* v_out, float* jt_out, float* scratch, size_t scratch_floats, fv_stream s);
/* the same on a prefix-width head (fv_head_set_flow_prefix): fusion.0.weight has prefix_chunk more columns behind phi(t), P is the flat buffer of THAT layout;
 * the chain runs with m = 0 and never reads the mask columns.  prefix_chunk >= 2 divides da. */
int fv_op_flow_vjp_prefix(int feat, int ds, int da, int hid, int fus, int time_dim, int prefix_chunk, const float* freq, const float* P, const float* pooled,
                          const float* states, int B, const float* x, float t, const float* omega, float* v_out, float* jt_out, float* scratch, size_t scratch_floats,
                          fv_stream s);
/* where fusion.0's input `cat` = [ pooled | state branch | x_t | phi(t) | m ] lies inside the saved activations (fv_head_saved_bytes) of a head with these
 * dimensions: *out_floats = its offset in floats; its shape is (draws * B, cat width).  time_dim 0: the regression head; draws 1 and prefix_chunk 0: off.
 * The layout is the library's own (csrc/head_kernels.hip carve): tests ask for it here instead of repeating it. */
int fv_op_head_saved_cat_offset(int feat, int ds, int da, int hid, int fus, int time_dim, int draws, int prefix_chunk, int B, size_t* out_floats);
/* the selection kernel of fv_head_flow_sample_multi alone, on candidates the test supplies: cand (S B, da) device f32, sample-major (row s B + b); select
 * FV_FLOW_SELECT_*; prev (B, da), shift, row_mask (B) int32 or NULL and step_w (chunk DEVICE floats) feed the coherence score; post_scale / post_shift (da)
 * device floats or both NULL: the action statistics `actions` folds in.  Outputs as fv_head_flow_sample_multi's: actions, chunk_out (B, da); optional
 * candidates_out (S B, da), choice_out (B) int32, scores_out (B, S), spread_out (B, da). */
int fv_op_flow_select(const float* cand, int B, int S, int da, int select, const float* prev, int shift, const int32_t* row_mask, const float* step_w, int chunk,
                      const float* post_scale, const float* post_shift, float* actions, float* chunk_out, float* candidates_out, int32_t* choice_out,
                      float* scores_out, float* spread_out, fv_stream s);

/* *flag_dev <- value (>= 0), stream-ordered: the step guard's sticky saturation flag (its address: fv_step_guard_flag in fastvla_hip.h) as saturating casts
 * followed by fv_step_guard_observe would leave it, without having to provoke a saturation. */
int fv_op_step_guard_set_flag(float* flag_dev, float value, fv_stream s);

#ifdef __cplusplus
}
#endif
#endif /* FASTVLA_HIP_TESTOPS_H */
