// kernels.h -- internal launch API shared by the engine (engine.hip) and the op-level C entry points (ops_api.hip).
// Every launcher validates the shapes its kernel and grid assume and returns an fv_status; nothing here allocates or
// synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fastvla_hip.h"
#include "../../include/fastvla_hip_testops.h"   // enum fv_gemm_epilogue (the fv_op_* declarations in it are test-only: ops_api.hip)
#include "common.h"

namespace fv {

struct GemmArgs {
  const bf16_t* A; int lda;     // [M,K] bf16
  const bf16_t* W;              // [N,K] bf16 (row stride K)
  int M, N, K;
  const float* bias;            // [N] or null
  const float* scale;           // [N] or null (FV_EPI_LS_RES)
  const void* res; int ldr;     // residual (bf16 for LS_RES, f32 for RES_F32) or null
  void* out; int ldo;           // bf16 or f32 by epilogue
  int epi;
  int ksplit = 0;               // 1: A holds [hi | lo] (2K columns, lda >= 2K); out = (hi + lo) . W^T in one launch
                                // 2: "hi + lo8": A rows = K bf16 then (at byte offset 2K) K fp8 remainders x 2^8 (lda >= 1.5 K); the lo product runs
                                //    against W8 on the scaled fp8 MFMA (K % 128 == 0); SWIGLU_SPLIT / fused-norm outputs leave in the same form
  int f16 = 0;                  // 1: A and W hold fp16 bits (v_mfma_f32_16x16x32_f16); not together with ksplit
  float* splitk_ws = nullptr;   // optional scratch for split-K partial sums (fp32 epilogues, few output tiles, long K)
  size_t splitk_bytes = 0;
  int lo_off = 0;               // FV_EPI_SWIGLU_SPLIT: column of the lo half in an output row (0 = N / 2).  launch_gemm's tail sub-launch (a column range of the
                                // problem) sets it to the whole problem's N / 2
  int no_tail = 0;              // 1: do not cut the last partial round of tiles off as a K-range sub-launch (set on the two sub-launches themselves)
  int few_rows = 1;             // 0: never the few-row K-range forms (64-row tiles x K ranges; the control loop's shapes).  The training path clears it: those
                                // forms add in another fp32 order, and a row's gradient must not depend on how many rows share its step
  // optional RMSNorm of the fp32 output rows (the decoder's next-layer input_layernorm): y (+ y_lo) = bf16 hi (+ lo) of
  // w * out * rsqrt(mean(out^2) + eps), row stride norm_ld; fused into the split-K reducer, a separate launch otherwise
  const float* norm_w = nullptr; bf16_t* norm_y = nullptr; bf16_t* norm_ylo = nullptr; int norm_ld = 0; float norm_eps = 0.f;
  const void* W8 = nullptr;     // ksplit == 2: fp8 e4m3 copy of W x 2^6, row stride 2K BYTES (the first K of each row valid: the bf16 copy's per-lane offsets serve both)
  unsigned* sat = nullptr;      // optional device counter: += 1 per 8-value group FV_EPI_SWIGLU_F16 had to clamp to the fp16 range
  void* stash = nullptr;        // FV_EPI_SWIGLU_SPLIT only: also keep the raw gate/up accumulators [M][N] (row stride N, the packed column order):
                                // what the SwiGLU backward of the unfrozen training path differentiates; fp32, or
  int stash_f16 = 0;            // 1: fp16 (saturating, clamps counted in *sat): half the bytes of a launch whose epilogue is write-bound
  // tn = 1 ("TN": the contraction runs over the ROWS of both operands, the wgrad's shape): A is [K][M] with row stride lda >= M, W is [K][N]
  // with row stride ldw >= N, out[m][n] = sum_k A[k][m] W[k][n].  K % 64 == 0 (rows past the data must be zero), M % 8 == 0, N % 8 == 0, fp32
  // epilogues, no ksplit; the 256-tile kernel only (LDS image in [k/8][n/16][8][16] blocks, fragments by ds_read_b64_tr_b16)
  int tn = 0, ldw = 0;
  const unsigned* skip = nullptr;   // prompt reuse (fv_set_prompt_reuse): device word; non-zero = every kernel of this launch returns at once.  null: as ever
};
int launch_gemm(const GemmArgs& a, hipStream_t s);

// What launch_gemm does with a problem.  plan_gemm makes every argument check and the whole routing decision for a device of `cus` CUs: no HIP call, no
// allocation, no state, and pointers are tested for null and alignment only; launch_gemm asks the device for `cus` and runs the plan.  One launch, or two where
// the tail is cut off (columns [c0, c1) each).  tests/gemm_util.py gemm_route mirrors it field for field (fv_op_gemm_plan is the tests' way in).
enum GemmReducer { GEMM_RED_NONE = 0, GEMM_RED_F32, GEMM_RED_NORM, GEMM_RED_NORM_ROW, GEMM_RED_BF16, GEMM_RED_SWIGLU };
enum GemmNorm { GEMM_NORM_NONE = 0, GEMM_NORM_FUSED, GEMM_NORM_SEPARATE };   // the RMSNorm of GemmArgs::norm_w: not asked, in the reducer, a launch of its own
struct GemmLaunch {
  int kernel;                                // row of gemm_bf16.hip's instance table (gemm_kernel_name)
  int tile;                                  // rows of a tile: 64 / 128 (the register-staged kernel; the pointwise kernel: 128), 128 / 256 (square)
  int tiles_n, tiles_m, tiles_mt, group_m;   // the tile walk, as the kernels' Params
  int splits, npad, nwg, grid;               // K ranges per tile (1: one pass), the partial sums' row stride, work units, blocks
  int reducer, norm;                         // GemmReducer (NONE: one pass), GemmNorm
  int c0, c1;                                // the launch's columns of the problem
};
struct GemmPlan { int n; GemmLaunch launch[2]; };
int plan_gemm(const GemmArgs& a, int cus, GemmPlan& plan);
const char* gemm_kernel_name(int kernel);     // "gemm256_kernel<8,4,ASYM,F16>": the spelling of tests/gemm_util.py
const char* gemm_reducer_name(int reducer);   // "" for GEMM_RED_NONE

// fused ConvFFN pointwise half: out = res + ls * (fc2(gelu(fc1(x) + b1)) + b2); w1 [4C][C] bf16, w2p = convffn_pack_w2 layout
bool convffn_supported(int C, int ratio);
void convffn_pack_w2(const float* w2, float* out, int C, int hidden);
int launch_convffn(const bf16_t* x, const bf16_t* w1, const float* b1, const bf16_t* w2p, const float* b2, const float* ls,
                   const bf16_t* res, bf16_t* out, int M, int C, int hidden, hipStream_t s);

// the same fused ConvFFN on v_mfma_f32_32x32x16_bf16 (convffn32.hip): C in {96, 192, 384}; wq = convffn32_pack stream (fc1 and
// fc2 weights, [4C/32 chunks][64 C elements])
bool convffn32_supported(int C, int ratio);
void convffn32_pack(const float* w1, const float* w2, float* out, int C);
int launch_convffn32(const bf16_t* x, const bf16_t* wq, const float* b1, const float* b2, const float* ls,
                     const bf16_t* res, bf16_t* out, int M, int C, int hidden, hipStream_t s, float* part = nullptr, size_t part_bytes = 0,
                     bf16_t* stash_y = nullptr);   // stash_y: [M][4C] fp16, the training forward's pre-activation / 4 (convffn32.hip STASH)
bool convffn32_stash_supported(int M, int C);

int launch_letterbox(const void* img, int dtype, int B, int C, int Hin, int Win, int S, float pad_value, int letterbox,
                     bf16_t* pix, hipStream_t s);
int launch_letterbox_norm(const void* img, int dtype, int B, int C, int Hin, int Win, int S, float pad_value, int letterbox, const float* mean3,
                          const float* std3, int range_heuristic, unsigned* vmax_scratch, bf16_t* pix, hipStream_t s);
// on-device image augmentation (augment_kernels.hip): the per-sample table drawn with Philox4x32-10, and the letterbox sampling through it
int launch_augment_draw(const fv_augment_config* cfg, const void* img, int dtype, int B, int C, int Hin, int Win, uint64_t seed, uint64_t offset,
                        uint64_t sample_base, fv_augment_sample* table, hipStream_t s);
int launch_letterbox_augmented(const void* img, int dtype, int B, int C, int Hin, int Win, int S, float pad_value, int letterbox,
                               const fv_augment_sample* table, float value_max, bf16_t* pix, hipStream_t s);
int launch_stem_conv(const bf16_t* pix, const float* w, const float* bias, bf16_t* y, int B, int S, int Cout,
                     hipStream_t s);
// implicit-GEMM stem on MFMA; wp = stem_mfma_pack image ([Cout][64] bf16), Cout % 16 == 0
void stem_mfma_pack(const float* w27, float* out, int Cout);
int launch_stem_mfma(const bf16_t* pix, const bf16_t* wp, const float* bias, bf16_t* y, int B, int S, int Cout, hipStream_t s);
// fused stem conv 3x3 s2 + GELU + depthwise 3x3 s2 + GELU: pix (B,S,S,4) -> y (B,S/4,S/4,96); C0 must be 96
bool stem_fused_supported(int S, int C0);
int launch_stem_fused(const bf16_t* pix, const bf16_t* wp, const float* b1, const float* w2, const float* b2, bf16_t* y, int B,
                      int S, int C0, hipStream_t s);
// the same stem sampling the SOURCE images (B,C,Hin,Win) f32 | u8 through the letterbox arithmetic: no (B,S,S,4) frame in HBM
int launch_stem_fused_lb(const void* img, int dtype, int B, int C, int Hin, int Win, float pad_value, int letterbox, const bf16_t* wp,
                         const float* b1, const float* w2, const float* b2, bf16_t* y, int S, int C0, hipStream_t s);
int launch_dwconv(const bf16_t* x, const float* w, const float* bias, bf16_t* y, int B, int H, int W, int C, int k,
                  int stride, int mult, int gelu, hipStream_t s);
// MFMA (4x4x4, 16 channel blocks) depthwise conv for stride-1 k in {3,7} on maps with W >= 32; ttab from dwconv_toeplitz_pack
bool dwconv_mfma_supported(int W, int C, int k, int stride, int mult);
size_t dwconv_toeplitz_elems(int C, int k);
void dwconv_toeplitz_pack(const float* w_tapmajor, float* out, int C, int k);
size_t dwconv_s2_toeplitz_elems(int C);
void dwconv_s2_toeplitz_pack(const float* w_tapmajor, float* out, int C);   // 7x7 stride 2, two outputs per input channel
bool dwconv_s2_mfma_supported(int H, int W, int C, int k, int stride, int mult);
int launch_dwconv_s2_mfma(const bf16_t* x, const bf16_t* ttab, const float* bias, bf16_t* y, int B, int H, int W, int C, int gelu,
                          hipStream_t s);
// x' = dw3x3(x), t = dw7x7(x') in one marching kernel (RepMixer token mixer + ConvFFN conv); tables as for launch_dwconv_mfma
bool dwconv_pair_supported(int B, int H, int W, int C);
int launch_dwconv_pair(const bf16_t* x, const bf16_t* t3, const float* b3, const bf16_t* t7, const float* b7, bf16_t* y1, bf16_t* y2,
                       int B, int H, int W, int C, hipStream_t s);
int launch_dwconv_mfma(const bf16_t* x, const bf16_t* ttab, const float* bias, bf16_t* y, int B, int H, int W, int C, int k,
                       int gelu, hipStream_t s);
int launch_layernorm_rows(const bf16_t* x, const float* w, const float* b, bf16_t* y, int rows, int C, float eps,
                          hipStream_t s);
int launch_se_gelu(const bf16_t* x, const float* w1, const float* b1, const float* w2, const float* b2, bf16_t* y,
                   float* scratch, int B, int P, int C, int R, hipStream_t s);
// lens (B) int32 or null; the visible key count of batch row b is clamp(lens[b] + len_add, 1, T)
int launch_attention(const bf16_t* q, const bf16_t* k, const bf16_t* v, int ldq, int ldk, int ldv, bf16_t* out,
                     int ldo, int B, int T, int heads, int kv_heads, int D, int causal, const int32_t* lens,
                     int len_add, float scale, hipStream_t s, const unsigned* skip = nullptr);   // skip: GemmArgs::skip (the causal / masked kernel only)

// decoder elementwise
int launch_embed_gather(const int32_t* ids, const bf16_t* table, const float* img_tokens, float* x, int B, int T,
                        int Ni, int H, int vocab, hipStream_t s, const unsigned* skip = nullptr);   // skip: as GemmArgs::skip, here and below
// y_lo != null: also writes the bf16 remainder (x ~= y + y_lo), the split operand of the parity-mode decoder GEMMs
int launch_rmsnorm(const float* x, const float* w, bf16_t* y, bf16_t* y_lo, int ldy, int rows, int H, float eps, hipStream_t s,
                   int f16 = 0, unsigned* sat = nullptr,    // f16 != 0: y receives fp16 bits (y_lo must be null), clamps counted in *sat
                   int lo8 = 0, const unsigned* skip = nullptr);   // lo8 != 0: the remainder leaves as fp8 (x 2^8), one byte per element, at y_lo's row starts
// in place: n bf16 values -> the fp16 values scale * x (weights of the fp16-operand projections, once at load time); maxbits (device,
// optional) receives max(|scale * x|) as float bits by atomicMax, so the loader can refuse weights outside the fp16 range
int launch_bf16_to_f16(bf16_t* p, size_t n, float scale, hipStream_t s, unsigned* maxbits = nullptr);
// W [rows][K] bf16 -> fp8 e4m3 copy of W x 2^6 at row stride 2K bytes (GemmArgs::W8); maxbits as launch_bf16_to_f16
int launch_bf16_to_w8(const bf16_t* w, void* w8, size_t rows, int K, hipStream_t s, unsigned* maxbits = nullptr);
int launch_rope_f32(float* qkv, const float2* table, int ld, int rows, int T, int heads, int kv_heads, int D, hipStream_t s, const unsigned* skip = nullptr);
// rope != null: qkv holds un-rotated projections; the rotate-half RoPE is fused into the MFMA kernel (head_dim 64 / 128) or applied
// in place by a rope_f32 launch ahead of the VALU kernel (head_dim 32)
int launch_attention_f32(float* qkv, int ld, bf16_t* out_hi, bf16_t* out_lo, int ldo, int B, int T, int heads,
                         int kv_heads, int D, const int32_t* lens, int len_add, float scale, hipStream_t s, const float2* rope = nullptr,
                         const float* pre = nullptr, int ldp = 0, int Np = 0,    // pre: cached [k | v] rows of positions < Np (8f-1)
                         float* lse = nullptr,    // optional [B][heads][T] row statistics max + log(sum) for the backward pass (head_dim 64 / 128, Np = 0)
                         int lo8 = 0,             // remainders as fp8 bytes (the hi + lo8 operand form of llm_precision = 5)
                         void* split_scratch = nullptr,    // attention_split_scratch_bytes() bytes -> the split-bf16 kernel (attention_split.hip) when lse is wanted (training)
                                                           // or the sequence is at least FV_ATTN_SPLIT_MIN_T long (the spliced prefill); never with a cached prefix or lo8
                         const unsigned* skip = nullptr);
constexpr int FV_ATTN_SPLIT_MIN_T = 128;
// table: [>=T][D/2] (cos, sin) pairs built by rope_table_host(); position = row % T
int launch_rope(bf16_t* qkv, const float2* table, int ld, int rows, int T, int heads, int kv_heads, int D,
                hipStream_t s, const unsigned* skip = nullptr);
void rope_table_host(float* cos_sin_pairs, int T, int D, float theta);
int launch_pool_norm(const float* x, const int32_t* lens, const float* w, float* pooled, int B, int Ttot, int Ni,
                     int H, float eps, int mode, hipStream_t s, const unsigned* skip = nullptr);

// ---- unfrozen-backbone training glue (train_kernels.hip) ------------------------------------------------------
constexpr int RMS_BWD_RPW = 4;      // rows per wave of rmsnorm_bwd_kernel (one dw partial row per wave)
constexpr int COLSUM_CHUNKS = 64;   // row ranges of the two-stage deterministic column sum
int launch_split_rows(const float* in, int ldi, bf16_t* out, int ldo, int lo_off, long R, int C, hipStream_t s);
int launch_lo8_rows(const float* in, int ldi, bf16_t* out, int ldo, long R, int C, hipStream_t s);   // the fp8 remainder bytes of the hi + lo8 operand form
int launch_bf16_to_f32(const bf16_t* in, float* out, size_t n, hipStream_t s);
int launch_transpose_to_bf16(const void* in, int in_bf16, int ldi, bf16_t* out, int ldo, int lo_off, int R, int Rp, int C, hipStream_t s);
// the same transpose to fp16 (saturating; clamps counted in *sat): in_kind 0 = fp32, 1 = bf16, 2 = split bf16 (value = in[c] + in[lo_in + c]: both halves summed before rounding), 3 = fp16
int launch_transpose_to_f16(const void* in, int in_kind, int ldi, int lo_in, bf16_t* out, int ldo, int R, int Rp, int C, unsigned* sat, hipStream_t s,
                            bf16_t* rows_out = nullptr, int ldro = 0);   // rows_out: the same values also as fp16 rows [R][ldro]
int launch_rows_to_f16(const void* in, int in_kind, int ldi, int lo_in, bf16_t* out, int ldo, long R, int C, unsigned* sat, hipStream_t s,
                       long Rp = 0);   // Rp > R: rows [R, Rp) of the output written as zeros (the TN wgrad's K-tile padding)   // row-major fp16 rows (in_kind as above)
int launch_swiglu_bwd(float* gu, const float* dact, long rows, int I, hipStream_t s, bf16_t* out_split = nullptr);   // out_split: [rows][4I] = [hi | lo] bf16 instead of fp32 in place
// dgu straight into the two fp16 operands of its consumers: rows [rows][2I] and columns [2I][Rp] (zero for rows in [rows, Rp)); clamps counted in *sat
// d gate/up and act as fp16 ROWS only, rows [rows, Rp) zero: the operands of the TN wgrads (and d gate/up's rows of the dgrad)
int launch_swiglu_bwd_rows(const void* gu, int gu_f16, const float* dact, long rows, long Rp, int I, bf16_t* dgu_rows, bf16_t* act_rows, unsigned* sat, hipStream_t s);
int launch_swiglu_bwd_f16(const void* gu, int gu_f16, const float* dact, int rows, int Rp, int I, bf16_t* out_rows, bf16_t* outT, unsigned* sat, hipStream_t s,
                          bf16_t* actT = nullptr);   // gu_f16: the kept accumulators are fp16 (GemmArgs::stash_f16)   // actT: also silu(gate) * up as fp16 columns [I][Rp] (the down projection's wgrad operand)
int launch_gelu_fwd(const float* pre, bf16_t* out, int ldo, int lo_off, long R, int C, hipStream_t s);
int launch_gelu_bwd(float* dh, const float* pre, size_t n, hipStream_t s);
size_t rmsnorm_bwd_scratch_floats(long rows, int H);
int launch_colsum(const float* in, int ld, long R, int C, float* out, float* scratch, hipStream_t s);   // scratch >= COLSUM_CHUNKS * C floats
int launch_rmsnorm_bwd(const float* x, const float* w, const float* dy, const float* dres, float* dx, float* dw, float* scratch, long rows, int H,
                       float eps, hipStream_t s);
int launch_pool_rows(float* stream, float* compact, const int32_t* lens, int B, int Tt, int Ni, int H, int scatter, hipStream_t s);
int launch_image_rows(const float* stream, float* compact, int B, int Tt, int Ni, int H, hipStream_t s);
int launch_embed_bwd(const int32_t* ids, const int32_t* lens, const float* dx, float* dE, int B, int T, int Ni, int H, int vocab, hipStream_t s);
int launch_attention_bwd(const float* qkv, int ld, const bf16_t* o_hi, const bf16_t* o_lo, int ldo, const float* dO, int lddo, const float* lse,
                         float* delta, float* dqkv, int B, int T, int heads, int kv_heads, int D, const int32_t* lens, int len_add, float scale,
                         const float2* rope, hipStream_t s, float* part = nullptr,    // part: optional scratch of (heads / kv_heads) * B * T * 2 * kv_heads * D floats
                         void* split_scratch = nullptr);   // attention_split_scratch_bytes() bytes -> the split-bf16 kernels (attention_split.hip)
                                                                                       // -> dK / dV per q head in parallel, then summed in a fixed order

// fv_train_commit in ONE launch: every trainable tensor of the flat fp32 master -> the library's operand copies.  One descriptor per tensor
// (device array, sorted by tile0); a block takes one 64 x 64 tile of a matrix (bf16 rows + the transposed dgrad copy, fp16 or bf16) or 4096
// floats of a vector
struct CommitDesc {
  long long src_off;     // offset into the flat master (floats)
  void* dst;             // bf16 [rows][cols] (matrix) or fp32 [numel] (vector)
  void* dstT16;          // fp16 [cols][rows] or null
  void* dstTb;           // bf16 [cols][rows] or null
  int rows, cols;        // vector: rows = 1, cols = numel
  int is_mat;
  int tile0;             // first tile of this tensor in the launch's tile numbering
  void* dst16;           // fp16 [rows][cols] copy x scale16 or null (the one-pass fp16 training forward's weight operand)
  float scale16;
};
int launch_commit(const CommitDesc* desc_dev, int ndesc, int ntiles, const float* flat, int f16_transposes, unsigned* sat, hipStream_t s);

// ---- LoRA mode of backbone training (lora_kernels.hip; fv_train_lora_*) ------------------------------------------------------------------
// one adapted LOGICAL matrix (q, k, v, o, gate, up or down of one layer): W' = W0 + s . B . A, A [rank][in], B [out][rank] in the trainable flat buffer
constexpr int LORA_STRIP_ROWS = 128;   // rows of dW' one block of the projection takes (dA leaves it as one partial sum per strip)
struct LoraMat {
  long long w_off;       // the PACKED tensor this matrix lives in: offset in the full flat buffer (master / gradient), floats; its row stride is `in`
  long long a_off, b_off;   // lora_A / lora_B in the trainable flat buffer (parameters and gradients alike), floats
  int out, in;           // logical rows x columns (multiples of 32)
  int row0, blk;         // logical row i = packed row row0 + (i >> 3) * blk + (i & 7)  (blk 8: plain or a q|k|v row range; 16: gate / up interleaved by 8)
  int strip0;            // first strip of this matrix in the projection's strip numbering
  long long part_off;    // its per-strip dA partial sums in the scratch, floats, relative to its launch group
  long long m_off, n_off;   // DoRA only: its magnitude vector (`out` floats) in the trainable flat buffer; its row norms in the handle's norm buffer
};
struct LoraCommitDesc {
  CommitDesc c;          // the packed tensor, as fv_train_commit sees it (tile0 in the LoRA launch's own numbering)
  int kind;              // 0 plain (mat[0]), 1 q|k|v row ranges (mat[0..2], qd / kd rows), 2 gate / up interleaved (mat[0] gate, mat[1] up)
  int qd, kd;
  int mat[3];            // index into the LoraMat table, -1 = that part has no adapter
  int band0;             // first 64-row band of this tensor in the row-norm launch's numbering (DoRA)
};
// dA, dB of matrices [m0, m1) (their strips: strip_begin .. strip_begin + nstrips) from ONE read of the full gradient; scratch holds the group's dA partials
// DoRA (W' = diag(m / n) (W0 + s . B . A), n the row norms of W0 + s . B . A, held constant in the backward): `norms` non-null selects it everywhere below.
// The projection then also needs the master (dm's row dot with W0) and leaves dm = (sum_j dW'_ij V_ij) / n_i beside dA = s B^T diag(c) dW', dB = s diag(c) dW' A^T.
int launch_lora_project(const LoraMat* mats_dev, int m0, int m1, int strip_begin, int nstrips, int max_in, const float* grads_full, const float* lora,
                        float* lora_grads, float* scratch, int rank, float scale, hipStream_t s, const float* master = nullptr, const float* norms = nullptr);
int launch_lora_commit(const LoraCommitDesc* desc_dev, int ndesc, int ntiles, const LoraMat* mats_dev, const float* flat, const float* lora, int rank, float scale,
                       int f16_transposes, unsigned* sat, hipStream_t s, const float* norms = nullptr);
int launch_lora_merge(const LoraCommitDesc* desc_dev, int ndesc, int ntiles, const LoraMat* mats_dev, float* flat, const float* lora, int rank, float scale,
                      hipStream_t s, const float* norms = nullptr);
// norms[n_off + i] = ||(W0 + s . B . A)_i,:||_2 of every adapted row (nbands = the tensors' 64-row bands); mag non-null: the magnitudes in that trainable buffer too
int launch_lora_norms(const LoraCommitDesc* desc_dev, int ndesc, int nbands, const LoraMat* mats_dev, const float* flat, const float* lora, int rank, float scale,
                      float* norms, float* mag, hipStream_t s);

// ---- the direct LoRA backward (lora_direct_kernels.hip; fv_train_lora_forward_backward): dA, dB straight from dY and X, dW' never formed --------------------
// ONE packed tensor of one layer and the adapters inside it ("slots", in part order: q, k, v / gate, up / the matrix itself)
struct LoraDirectPack {
  int kind;              // 0 plain, 1 q|k|v column ranges of dY (qd / kd wide), 2 gate / up interleaved by 8 (as LoraCommitDesc::kind)
  int nm, r, NCp;        // adapters in this call (1 .. 3), rank, nm * r rounded up to 32 (the width of the P / Q arrays)
  int Np, K;             // columns of dY (the packed tensor's rows) and of X (its columns); multiples of 32
  int qd, kd;
  int slot_of_part[3];   // part (0 q / gate / plain, 1 k / up, 2 v) -> slot, -1 = that part is not a target
  long long a_off[3], b_off[3];   // per slot: lora_A / lora_B in the trainable flat buffer (parameters and gradients alike), floats
};
size_t lora_direct_scratch_floats(long R, int rank, int max_cols);   // P | Q | partial sums for R rows; max_cols = the widest of any call's Np and K
// dY: fp16 rows [R][Np].  X: xkind 2 = split bf16 rows (value = X[c] + X[lo_off + c]), 3 = fp16 rows; row stride ldx.  lgrads receives s . dA, s . dB of every slot
int launch_lora_direct(const LoraDirectPack& pk, const bf16_t* dY, const bf16_t* X, int xkind, int ldx, int lo_off, int R, const float* lora, float* lgrads,
                       float scale, float* scratch, size_t scratch_floats, hipStream_t s);

// ---- tower backward (tower_bwd_kernels.hip; SURVEY.md 8f-4, second slice) ---------------------------------------------------------
// gradients NHWC fp16 (loss-scaled), activations NHWC bf16, weight gradients fp32 by fixed-order partial sums (no atomics)
size_t dw_bwd_scratch_floats(int B, int Ho, int Wo, int Co, int k);
int launch_dw_dgrad(const bf16_t* dy, const float* w, const bf16_t* res, bf16_t* dx, int B, int Hi, int Wi, int Ci, int k, int stride, int mult, unsigned* sat,
                    hipStream_t s, int round_w = 0);   // round_w: taps rounded to bf16 first (the forward ran on a bf16 Toeplitz table)
// the same input gradient on the marching MFMA depthwise kernel (stride 1, W >= 16, H >= 16, C % 32 == 0): ttab16 = fp16 Toeplitz table of the flipped taps
bool dw_dgrad_mfma_supported(int H, int W, int C, int k);
int launch_dw_dgrad_mfma(const bf16_t* dy, const bf16_t* ttab16, const bf16_t* res, bf16_t* dx, int B, int H, int W, int C, int k, unsigned* sat,
                         hipStream_t s);   // sat: counts the (pixel, 8-channel group) cells that clamp, as launch_dw_dgrad's does (may be null)
int launch_dw_wgrad(const bf16_t* x, const bf16_t* dy, float* dw, float* db, float* scratch, int B, int Hi, int Wi, int Ci, int k, int stride, int mult,
                    hipStream_t s);
constexpr int TOWER_COLSUM_CHUNKS = 512;   // row ranges of the tower backward's column sums (10^5 .. 10^6 rows of 96 .. 1536 columns: the grid must fill the chip)
int launch_colsum16(const bf16_t* in, int ld, long R, int C, float* out, float* scratch, hipStream_t s);   // scratch >= TOWER_COLSUM_CHUNKS * C floats
int launch_mul16(const bf16_t* a, const bf16_t* b, bf16_t* out, size_t n, unsigned* sat, hipStream_t s);
int launch_gelu_grad_mul(const bf16_t* dh, const bf16_t* pre, bf16_t* out, size_t n, unsigned* sat, hipStream_t s);   // out f16 = dh f16 * gelu'(pre bf16)
int launch_f16_to_f32(const bf16_t* in, float* out, size_t n, float scale, hipStream_t s);
int launch_scale_to_f16(const float* in, bf16_t* out, size_t n, float scale, unsigned* sat, hipStream_t s);   // out f16 = in * scale (saturating)
int launch_rescale_to_f16(const float* in, bf16_t* out, size_t n, float target, unsigned* bits, float* sc, unsigned* sat, hipStream_t s,
                          const float* target_mul_dev = nullptr);   // the tower's own gradient scale (device-chosen power of two)
int launch_unscale_dev(float* p, size_t n, const float* sc, hipStream_t s);
int launch_ones_col(bf16_t* out, int ld, int C, long R, hipStream_t s);   // fp16 rows [R][ld]: columns [C, C + 8) <- {1, 0, ..., 0}
int launch_ls_grads(const float* dWraw, const float* dbraw, const bf16_t* W, const float* bias, const float* ls, float* dW, float* db, float* dls, int C, int Kd,
                    hipStream_t s);
size_t ln_bwd_scratch_floats(long rows, int C);
int launch_ln_bwd(const bf16_t* x, const bf16_t* dy, const float* w, const bf16_t* res, bf16_t* dx, float* dw, float* db, float* scratch, long rows, int C,
                  float eps, unsigned* sat, hipStream_t s);
int launch_tower_attn_bwd(const bf16_t* qkv, int ld, const bf16_t* dO, int lddo, bf16_t* dqkv, int ldd, float* stats, int B, int T, int heads, float scale,
                          hipStream_t s);   // stats: 2 * B * heads * T floats
int launch_se_bwd(const bf16_t* e, const bf16_t* dout, const float* se, const float* w1, const float* w2, bf16_t* de, float* dW1, float* db1, float* dW2,
                  float* db2, float* tmp, int B, int P, int C, int R, unsigned* sat, hipStream_t s);   // tmp >= B * (2 C + 2 R) floats
size_t stem0_wgrad_scratch_floats(int B, int S, int C0);
int launch_stem0_wgrad(const bf16_t* pix, const float* w, const float* bias, const bf16_t* dh0, float* dw, float* db, float* scratch, int B, int S, int C0,
                       hipStream_t s, int round_w = 0);
// fp16 patch rows of the stem's dense 3x3 s2 conv: P [B (S/2)^2][32], column (ky*3+kx)*3+ci, column 27 = 1 (the bias tap), 28 .. 31 = 0
int launch_stem_im2col16(const bf16_t* pix, bf16_t* P, int B, int S, hipStream_t s);
// fv_train_commit's tower part: one launch over a table of operations (device array, sorted by blk0; a block = 1024 destination elements)
//   kind 0: dst f32[i] = src[i]      1: dst bf16[i] = src[i]      2: dst bf16[i] = idx[i] >= 0 ? coef[i] * src[idx[i]] : 0   (the packed operand images)
//   kind 3: dst f16 [cols][rows] = src[rows][cols]^T              4: the same with row r scaled by flat[src2_off + r]         (dgrad operands)
//   kind 5: as 2 with the value rounded to bf16 first and stored as fp16 (the flipped-tap Toeplitz tables of the depthwise input gradients)
struct TowerCommitOp {
  long long src_off, src2_off, n;
  void* dst;
  const int* idx; const float* coef;
  int kind, rows, cols, blk0;
};
int launch_tower_commit(const TowerCommitOp* ops_dev, int nops, int nblocks, const float* flat, unsigned* sat, hipStream_t s);

// attention_split.hip: the same forward (training: with lse) and backward on the bf16 matrix core with split (hi + lo) operands, three passes per product
// scratch: attention_split_scratch_bytes(B, T, kv_heads, D) bytes -- K (rotated) and V of every kv head as split bf16 in both operand forms, written once
// per call by a small pre-pass and copied flat into LDS by every q head's / query block's thread block
size_t attention_split_scratch_bytes(int B, int T, int kv_heads, int D);
int launch_attention_split_fwd(const float* qkv, int ld, bf16_t* out_hi, bf16_t* out_lo, int ldo, int B, int T, int heads, int kv_heads, int D,
                               const int32_t* lens, int len_add, float scale, const float2* rope, float* lse, void* scratch, hipStream_t s,
                               const unsigned* skip = nullptr);
int launch_attention_split_bwd(const float* qkv, int ld, const bf16_t* o_hi, const bf16_t* o_lo, int ldo, const float* dO, int lddo, const float* lse,
                               float* delta, float* dqkv, int B, int T, int heads, int kv_heads, int D, const int32_t* lens, int len_add, float scale,
                               const float2* rope, hipStream_t s, float* part, long pstride, void* scratch);

// action expert (all fp32)
// flow mode (fv_head_set_flow): fusion.0 reads te + da more columns, cat = [ pooled | state branch | x_t (da) | phi(t) (te) ]; te == 0: the regression head
// draws (fv_head_set_flow_draws, flow mode only): S noise draws per observation in the training forms.  Head rows are draw-major, r = s B + b: the state branch
// keeps B rows, everything from cat on has S B.  1: the head as ever
// prefix mode (fv_head_set_flow_prefix, flow mode only): pk = K > 0 mask columns m behind phi(t), m[k] = 1 for the k < d steps of the chunk that are given to
// the network clean (d <= pd = D, the largest delay); `saved` also keeps the (head rows, K) byte mask the loss reads.  pk == 0: the flow head as ever
// bins mode (fv_head_set_bins, never together with flow mode): nb > 0 logits per action element -- action_head is (da nb, fus), the logits (head rows, da, nb)
// are kept in `saved`, what the callers see as actions stays (head rows, da): the decoded chunk.  bn: the mode's configuration, non-null exactly when nb > 0
struct HeadBins { const float* range; int n_range; float sigma; int decode; };   // range: device [lo | hi | w], n_range floats each; element e reads entry e % n_range
struct HeadDims { int feat, ds, da, hid, fus; int te = 0; int draws = 1; int pk = 0; int pd = 0; int nb = 0; const HeadBins* bn = nullptr; };
inline int head_out_width(const HeadDims& d) { return d.nb > 0 ? d.da * d.nb : d.da; }   // rows of action_head.weight
inline int head_cat_width(const HeadDims& d) { return d.feat + d.hid + (d.te > 0 ? d.da + d.te + d.pk : 0); }
inline int head_rows(const HeadDims& d, int B) { return d.te > 0 && d.draws > 1 ? d.draws * B : B; }
// the 12 parameter tensors in the flat buffer's order (head_offsets; fv_head_layout's offsets[13] and Python's head_views are the same order), then the total
enum HeadParam {
  HP_STATE_LN_W, HP_STATE_LN_B,   // state_projection.0 (LayerNorm)
  HP_STATE_W, HP_STATE_B,         // state_projection.1 (Linear, then SiLU)
  HP_FUS0_W, HP_FUS0_B,           // fusion.0 (Linear over cat)
  HP_FUS_LN_W, HP_FUS_LN_B,       // fusion.1 (LayerNorm, then SiLU and dropout)
  HP_FUS4_W, HP_FUS4_B,           // fusion.4 (Linear, then SiLU)
  HP_ACT_W, HP_ACT_B,             // action_head
  HP_TOTAL                        // o[HP_TOTAL]: the flat buffer's length in floats; also the number of tensors
};
struct HeadOffsets { int64_t o[HP_TOTAL + 1]; };
HeadOffsets head_offsets(const HeadDims& d);
size_t head_saved_bytes(const HeadDims& d, int B);
size_t head_saved_cat_offset(const HeadDims& d, int B);   // floats from the start of `saved` to its (head_rows(d, B), head_cat_width(d)) matrix `cat` (the test-only ops hand it out)
// (the two launchers that only the head's own translation units call stay out of the library's dynamic symbol table)
__attribute__((visibility("hidden"))) uint8_t* head_saved_prefix_mask(const HeadDims& d, int B, float* saved);   // prefix mode: the (head_rows(d, B), pk) byte mask inside `saved`, 1 = the step is conditioned on and does not train
__attribute__((visibility("hidden"))) float* head_saved_cat(const HeadDims& d, int B, float* saved);   // the (head_rows(d, B), head_cat_width(d)) matrix `cat` inside `saved` (launch_flow_prepare writes its x_t and phi(t) columns)
inline unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }   // grid sizes of the head, chunk, flow and optimiser launchers
// dataset normalisation folded into the head (device vectors; LeRobot MEAN_STD): states <- (states - state_mean) * state_istd
// ahead of the first LayerNorm; actions <- actions * action_std + action_mean behind the last Linear when not training
struct HeadIoNorm { const float *state_mean, *state_istd, *action_mean, *action_std; };
int launch_head_forward(const HeadDims& d, const float* P, const float* pooled, const float* states, int B,
                        int training, float drop_p, uint64_t seed, uint64_t offset, float* actions, float* saved,
                        hipStream_t s, const HeadIoNorm* io = nullptr);
// the state branch alone (two launches; no checks, no error query: its callers do both): n0 = LN((states - state_mean) * state_istd) with xh0 / rstd0 kept,
// z1 = state_projection.1(n0), dst[b][0 : hid] = silu(z1[b]) with row stride ldd.  launch_head_forward writes cat[:, feat:], the samplers a buffer of their own
__attribute__((visibility("hidden"))) void launch_head_state_branch(const HeadDims& d, const float* P, const float* states, int B, float* n0, float* xh0, float* rstd0, float* z1, float* dst,
                                                                   int ldd, hipStream_t s, const HeadIoNorm* io);
// the fused loss of launch_head_backward (fv_head_set_loss / fv_head_set_loss_mask): kind FV_LOSS_*, beta of smooth-L1, chunk = K steps of da / K action
// dimensions each, pad = device (B, K) bytes or null, metrics = 2 device floats { masked MSE, valid fraction }.  null, or MSE without a mask: mse_kernel as ever
// dim_w (da / chunk floats) and step_w (chunk floats): device vectors of fv_head_set_loss_weights, both set or both null.  Set: EVERY kind, plain MSE without a
// mask included, takes the chunked kernel's weighted instance
struct HeadLoss { int kind; float beta; int chunk; const uint8_t* pad; float* metrics; const float* dim_w = nullptr; const float* step_w = nullptr; };
// grad_actions != null: generic backward from dL/dactions (loss untouched); else fused MSE(actions, targets) + backward
// d_pooled (optional, [B][feat]): dL/d(pooled feature) -- the gradient an UNFROZEN backbone continues from
int launch_head_backward(const HeadDims& d, const float* P, const float* grad_actions, const float* actions,
                         const float* targets, int B, float drop_p, const float* saved, float* loss, float* G,
                         float* scratch, hipStream_t s, float* d_pooled = nullptr, float loss_scale = 1.0f,    // loss_scale: the fused loss's dL/dactions times a power of two
                         const struct HeadLoss* hl = nullptr,
                         const float* ga_scale_dev = nullptr);   // the step guard's dynamic factor (fv_train_set_step_guard): the fused loss's dL/dactions times *ga_scale_dev, one axpy launch
size_t head_bwd_scratch_bytes(const HeadDims& d, int B);
// ---- binned action head (bins_kernels.hip).  logits, g (n, nb) f32 with n = rows * da groups; targets (n) continuous; pad (n / (da / K)) bytes or null;
// partial: bins_loss_partial_floats(n) floats of scratch; loss 1 float; metrics 4 floats { decoded squared error / n, valid / n, hits / valid, 0 }
size_t bins_loss_partial_floats(long n);
int launch_bins_loss(const HeadBins& hb, const float* logits, const float* targets, const uint8_t* pad, float* g, float* partial, float* loss, float* metrics, long n,
                     int nb, int da, int K, float loss_scale, hipStream_t s, const float* dim_w = nullptr, const float* step_w = nullptr);
// logits -> actions (n; null: none, probs is required then) by hb.decode, then actions * post_scale[e] + post_shift[e] (da floats each, both or neither); probs (n, nb) or null: softmax(logits) too
int launch_bins_decode(const HeadBins& hb, const float* logits, float* actions, float* probs, long n, int nb, int da, const float* post_scale, const float* post_shift,
                       hipStream_t s);
__attribute__((visibility("hidden"))) float* head_saved_logits(const HeadDims& d, int B, float* saved);   // bins mode: the (head_rows(d, B), da, nb) logits inside `saved`
// ---- flow-matching head (d.te > 0).  freq: te / 2 device floats, 2 pi / period_j.  time_dist 0: t ~ U[0, 1); 1: t = sigmoid(dist_a + dist_b n)
// thr (prefix mode): pd + 1 device uint32, the cumulative delay distribution in units of 2^-24 (the last one is 2^24)
// FlowTime (fv_head_set_flow_time; on == 0: the handle draws t as fv_head_set_flow says): t = t_lo + (t_hi - t_lo) F^-1(u) from the one uniform of the row.
// dist 0 uniform, 1 logit-normal, 2 Beta(a, b); lbeta = log B(a, b), formed once on the host in double (dist 2 only)
struct FlowTime { int on = 0, dist = 0, stratify = 0; float a = 0.f, b = 0.f, t_lo = 0.f, t_hi = 1.f; double lbeta = 0.0; };
struct HeadFlow { const float* freq; int time_dist; float dist_a, dist_b; const uint32_t* thr = nullptr; FlowTime tm = {}; };
// one launch: draws (or reads) t per row and noise per element, writes x_t and phi(t) into their columns of saved's cat and u = noise - targets into u_out.
// d.draws = S > 1: targets (B, da) stay per observation; head row s B + b draws what row b draws at offset + (s << 56); noise, t and u_out have S B rows.
// FV_ERR_ARG, nothing enqueued, when S > 1 and any of bits 56 .. 59 of the offset is set
// prefix mode (d.pk > 0): the kernel's PREFIX instance -- row r's delay is delays[r] clamped to 0 .. pd (device int32, S B of them) or, with delays == null, drawn from
// word z of the group-0 Philox block that yields t; the first d steps of x_t are COPIES of targets, m and the row's byte mask in `saved` are written too
int launch_flow_prepare(const HeadDims& d, const HeadFlow& f, const float* targets, int B, uint64_t seed, uint64_t offset, const float* noise, const float* t,
                        float* saved, float* u_out, hipStream_t s, const int32_t* delays = nullptr);
// the sampler: conditioning once, then three launches per network evaluation.  scratch: flow_sample_scratch_bytes(d, B)
// pin != null: the prefix sampler (d.pk > 0).  Row b's first min(delays[b], pd, pk - shift) steps are pinned to prev[b][k + shift] (normalised) from the start
// to the end, and the mask block of fusion.0 joins c once per call: the same launches and scratch, the PREFIX instances of three kernels.  chunk_out (B, da)
// or null: the final normalised x_0
struct FlowPin { const float* prev; const int32_t* delays; int shift; float* chunk_out; };
size_t flow_sample_scratch_bytes(const HeadDims& d, int B);
int launch_flow_sample(const HeadDims& d, const HeadFlow& f, const float* P, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                       uint64_t seed, uint64_t offset, float* actions, float* scratch, hipStream_t s, const HeadIoNorm* io, int solver = 0, float* rk_rows = nullptr,
                       const FlowPin* pin = nullptr);
// several samples per observation (fv_head_set_flow_samples / fv_head_flow_sample_multi): S candidates, head rows sample-major (r = s B + b), candidate s the
// single-sample call at offset + (s << 56); then ONE of them is chosen per observation on the device (flow_select_kernels.hip).  mode FV_FLOW_SELECT_*;
// prev (B, da) normalised, shift, row_mask (B) int32 or null, step_w (chunk device floats >= 0): the coherence score's, all unused by the other modes;
// actions, chunk_out (B, da); optional candidates_out (S B, da), choice_out (B), scores_out (B, S), spread_out (B, da).
// scratch: flow_multi_scratch_bytes(d, S B); rk_rows: flow_rk_scratch_bytes(d, S B)
struct FlowSelect {
  int mode; const float* prev; int shift; const int32_t* row_mask; const float* step_w; int chunk;
  float *actions, *chunk_out, *candidates_out; int32_t* choice_out; float *scores_out, *spread_out;
};
size_t flow_multi_scratch_bytes(const HeadDims& d, int R);
int launch_flow_sample_multi(const HeadDims& d, const HeadFlow& f, const float* P, const float* pooled, const float* states, int B, int S, int n_steps,
                             const float* noise, uint64_t seed, uint64_t offset, float* scratch, hipStream_t s, const HeadIoNorm* io, int solver, float* rk_rows,
                             const FlowPin* pin, const FlowSelect& sel);
// the selection alone, on candidates (S B, da) the caller supplies: flow_select_check refuses (nothing enqueued), launch_flow_select checks and launches.
// post_scale / post_shift (da) or null: the action statistics `actions` folds in
__attribute__((visibility("hidden"))) int flow_select_check(const FlowSelect& sel, int S, int da);
int launch_flow_select(const float* cand, int B, int S, int da, const FlowSelect& sel, const float* post_scale, const float* post_shift, hipStream_t s);
// the integrators (fv_head_set_flow_solver), for all three samplers: solver = FV_FLOW_SOLVER_*, n_steps x stages evaluations whose x update is a Runge-Kutta
// stage.  Euler has one stage and needs nothing more; the others work over rk_rows: two more (B, da) rows, the step's start x0 and the running sum S,
// flow_rk_scratch_bytes(d, B) in all.  FV_ERR_ARG for an unknown solver, FV_ERR_STATE without the rows
size_t flow_rk_scratch_bytes(const HeadDims& d, int B);
// guided sampling (fv_head_set_flow_guidance): step_w = chunk device floats >= 0, beta the largest guidance weight, live_steps = 1 + the last step whose
// weight is not 0 (0: none).  prev (B, da): the previous chunk, normalised; Y[b][k] = prev[b][k + shift]; row_mask (B) int32 or null; chunk_out (B, da) or null:
// the final normalised x_0.  A row with all-zero omega comes out as launch_flow_sample's row, bit for bit.  scratch: flow_guided_scratch_bytes(d, B)
struct HeadGuide { const float* step_w; int chunk; float beta; int live_steps; };
size_t flow_guided_scratch_bytes(const HeadDims& d, int B);
int launch_flow_sample_guided(const HeadDims& d, const HeadFlow& f, const HeadGuide& gd, const float* P, const float* pooled, const float* states, int B, int n_steps,
                              const float* noise, uint64_t seed, uint64_t offset, const float* prev, int shift, const int32_t* row_mask, float* actions,
                              float* chunk_out, float* scratch, hipStream_t s, const HeadIoNorm* io, int solver = 0, float* rk_rows = nullptr);
// one guided step's forward and backward chain for given x (B, da), t and omega (B, da): v_out = v(x, t), jt_out = (dv / dx)^T omega.  Same scratch
int launch_flow_vjp(const HeadDims& d, const HeadFlow& f, const float* P, const float* pooled, const float* states, int B, const float* x, float t,
                    const float* omega, float* v_out, float* jt_out, float* scratch, hipStream_t s);
// the chunked loss alone (what launch_head_backward runs when HeadLoss asks for it): a, t, g (n) f32, pad (n / A) bytes or null, partial
// chunk_loss_partial_floats() floats of scratch, loss 1 float, metrics 2 floats
size_t chunk_loss_partial_floats();
int launch_chunk_loss(const float* a, const float* t, const uint8_t* pad, float* g, float* partial, float* loss, float* metrics, long n, int A, int kind,
                      float beta, float loss_scale, hipStream_t s, const float* dim_w = nullptr, const float* step_w = nullptr, int K = 1,
                      int prefix = 0);   // prefix != 0: a pad byte of 2 marks a step masked by the action prefix alone -- masked like a padded one, but counted as valid
// mean |a - t| per action dimension over the non-padded steps: a, t (rows, A) f32 with rows = B K, pad (rows) bytes or null -> out (A), 0 for a dimension
// without a valid step.  One block per dimension, fixed-order sums
// pad_rows (0: rows): the mask has fewer rows than a, t and row r reads pad[r % pad_rows] -- the draws of a flow head share their observation's mask
int launch_loss_per_dim(const float* a, const float* t, const uint8_t* pad, float* out, long rows, int A, hipStream_t s, long pad_rows = 0);
// the squared error by time bucket (fv_head_loss_per_time): a, u (R, da) f32, t (R), pad (B, K) bytes or null (row r reads the mask of observation r % B) ->
// out (nb, 2): { sum of (a - u)^2 over the non-padded elements of the rows in the bucket, their number }.  One block per bucket, fixed-order sums
int launch_loss_per_time(const float* a, const float* u, const float* t, const uint8_t* pad, float* out, int R, int B, int da, int K, int nb, hipStream_t s);
// temporal ensembling of action chunks (fv_ensemble_step): chunks (n_env, K, A) -> actions (n_env, A); ens (n_env, K, A) and count (n_env, K) are the ring,
// head its position, w / cw the K weights exp(-coeff i) and their running sums
int launch_ensemble_step(const float* chunks, float* ens, int32_t* count, float* actions, const float* w, const float* cw, int n_env, int K, int A, int head,
                         hipStream_t s);
size_t adamw_scratch_bytes();  // norm_scratch of launch_adamw_clip: [0] = sum of squares, [1..] per-block partials
int launch_axpy(float* y, const float* x, int64_t n, const float* scale_dev, hipStream_t s);  // y += x, or y *= *scale_dev when x is null
// ema != null (both launchers): the EMA instance of the step kernel, ema <- ema + ema_weight (p_new - ema) in the same pass (common.h ema_update);
// FV_ERR_ARG when ema overlaps another operand or ema_weight is outside [0, 1].  ema_weight == 0 runs the plain instance: ema is not touched.
int check_adamw_ema(const char* who, const float* p, const float* g, const float* m, const float* v, const float* ema, float ema_weight, int64_t n);
int launch_adamw_clip(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp,
                      int64_t step, float* norm_scratch, float* grad_norm_out, hipStream_t s, float* ema = nullptr, float ema_weight = 0.f);

// parameter groups of the fused step (optim_kernels.hip).  The host cuts every group into segments of at most FV_ADAMW_SEGMENT floats: a segment never
// straddles a group, every boundary is a multiple of 4 floats, the segments of a group are consecutive.  One block per segment in every kernel.
struct AdamwSeg { int64_t begin; int32_t len, group; };                                                   // 16 bytes
struct AdamwGroupDev { float lr_scale, weight_decay; int32_t frozen, seg_begin, seg_count, pad[3]; };     // 32 bytes
struct AdamwGroupsTable {
  const AdamwSeg* segs; const AdamwGroupDev* groups;   // device
  float* sums;                                         // device: [n_segs] segment partials | [n_groups] group sums | [1] total over the non-frozen groups
  int64_t n; int n_groups, n_segs;
};
int launch_adamw_clip_groups(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp, const AdamwGroupsTable& t,
                             int64_t step, float* grad_norm_out, float* group_norms_out, hipStream_t s, float* ema = nullptr, float ema_weight = 0.f);

// the step guard (fv_step_guard, optim_kernels.hip): its whole state is this one device block.  delta = 2^delta_log2 is what the training backward multiplies
// dL/dactions by (launch_head_backward's ga_scale_dev points at it); apply / inv_delta are the last decision, read by every block of the GUARD step kernels
struct GuardWords {
  int32_t delta_log2, good_steps, apply; float inv_delta;   // inv_delta: 2^-delta_log2 of the step the decision was made for
  float flag; uint32_t last_sat; float delta; int32_t pad;  // flag: sticky, > 0 when the saturation counter moved since the last guarded step
  unsigned long long applied, skipped_nonfinite, skipped_saturated, saturated_applied;
};                                                          // 64 bytes
struct GuardCfg { int32_t min_log2, max_log2, growth_interval, backoff_log2, growth_log2, skip_on_saturation; };
int launch_guard_observe(GuardWords* w, const unsigned* sat_counter, hipStream_t s);
int launch_guard_report(const GuardWords* w, float* out2, hipStream_t s);   // out2 <- { 1 - apply of the last decision, delta of the next backward }
// guard != null versions of the two steps: sums of squares by the same kernels, ONE decision launch (one block), then the GUARD instance of the step kernel
int launch_adamw_clip_guarded(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp, int64_t step, float* norm_scratch,
                              float* grad_norm_out, hipStream_t s, float* ema, float ema_weight, GuardWords* guard, const GuardCfg& cfg);
int launch_adamw_clip_groups_guarded(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp, const AdamwGroupsTable& t, int64_t step,
                                     float* grad_norm_out, float* group_norms_out, hipStream_t s, float* ema, float ema_weight, GuardWords* guard, const GuardCfg& cfg);

}  // namespace fv
