/*
 * fastvla_hip.h -- C ABI of libfastvla_hip.so: the MI355X-native (gfx950) FastVLA policy-step hot path.
 *
 * The reference (syun88/VLA-from-FastVLM) has NO FFI: its boundary is Python-level.  Each entry point below cites the
 * reference function whose arithmetic it replaces (paths relative to the reference root).  The only caller is the
 * host-side mirror in vla-from-fastvlm_amd/ (ctypes); tensors cross the boundary as raw device pointers + sizes.
 *
 * Conventions
 *   - return 0 on success, negative fv_status on error; message via fv_last_error(); never throws, never exits.
 *   - a handle is bound to ONE device; one handle per rank/process; calls are asynchronous on the supplied stream;
 *     no hidden hipDeviceSynchronize, no allocation inside forward/backward calls (graph-capturable).
 *   - caller owns inputs, outputs, trainable parameters, optimizer state and the workspace; the library owns only
 *     the packed frozen weights.
 *   - activations: NHWC bf16 in the tower, [tokens][hidden] f32 residual stream in the decoder.
 */
#ifndef FASTVLA_HIP_H
#define FASTVLA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fv_handle fv_handle;
typedef void* fv_stream; /* hipStream_t */

enum fv_status {
  FV_OK = 0,
  FV_ERR_ARG = -1,       /* bad argument / shape (reference: ValueError, fastvlm_adapter.py:41-42,150-154) */
  FV_ERR_STATE = -2,     /* weights/workspace missing (reference: RuntimeError, fastvlm_adapter.py:366-367,556) */
  FV_ERR_HIP = -3,       /* HIP runtime error */
  FV_ERR_MISSING = -4,   /* a required weight tensor was not supplied */
  FV_ERR_UNSUPPORTED = -5
};

enum fv_dtype { FV_F32 = 0, FV_BF16 = 1, FV_U8 = 2, FV_I32 = 3 };

#define FV_MAX_STAGES 8

typedef struct fv_model_desc {
  /* Qwen2 decoder ([site] transformers/models/qwen2/modeling_qwen2.py) */
  int32_t llm_hidden, llm_layers, llm_heads, llm_kv_heads, llm_head_dim, llm_inter, llm_vocab;
  float rope_theta, rms_eps;
  /* FastViT-HD tower ([UNVENDORED] mci.py `fastvithd`) */
  int32_t tower_stages;
  int32_t tower_layers[FV_MAX_STAGES];
  int32_t tower_dims[FV_MAX_STAGES];
  int32_t tower_is_attn[FV_MAX_STAGES];
  int32_t tower_mlp_ratio, tower_head_dim, tower_se_rd; /* se_rd = int(out_dim * 0.0625) */
  int32_t tower_out_dim;                                 /* 2 * dims[last] */
  float ln_eps, bn_eps;
  int32_t image_size;                                    /* S: square side the tower runs at (expected_size) */
  /* action expert (fastvla/fastvlm_with_expert.py:23-38) */
  int32_t state_dim, action_dim, hidden_dim, fusion_dim;
  /* capacity */
  int32_t max_batch, max_text_tokens;
  int32_t tower_microbatch; /* images per tower pass (0 = whole batch) */
  /* decoder arithmetic: 0 = bf16 MFMA operands (fastest; actions ~8e-3 from the fp32 reference at 0.5B),
   * 1 = split-bf16 activations (hi + lo, two MFMA passes, exact bf16 weights) + fp32 attention: 16 significant bits on
   * every GEMM operand, actions within 1e-3 of the fp32 reference (the parity bar of north_star).  Tower unaffected.
   * 2 = the per-GEMM budget of tests/precision_budget.py: qkv and o keep split-bf16 operands (12 % of the decoder's MACs), gate/up
   * and down run ONE pass on fp16 operands (11 significant bits; fp16 copies of those weights are exact for |w| >= 6e-5 and the
   * down projection carries a 2^4 scale against a 2^-4 on its operand), fp32 attention: actions ~5e-4 from the fp32 reference at
   * 0.56x the MFMA work of mode 1.  3 / 4 = the two halves of mode 2 on their own (3: the fp16 pass on gate/up only, its SwiGLU output
   * leaves as hi + lo bf16 for a split-bf16 down projection; 4: on down only): the per-family rows of the precision budget measured on
   * the product (tools/prec_sweep.py), not defaults of any preset.
   * 5 = "hi + lo8" (round 4): every split operand keeps its bf16 hi half and carries the remainder as ONE fp8 e4m3 byte (x 2^8); the lo product
   * runs on v_mfma_scale_f32_16x16x128_f8f6f4 against fp8 copies of the weights (x 2^6) at twice the bf16 MFMA rate: 1.5 passes instead of 2,
   * 13 significant bits per operand instead of 16 (5.8e-5 per GEMM; split-bf16 2.5e-6, one fp16 pass 2.1e-4); fp32 attention.  Needs hidden,
   * inter and heads * head_dim % 128 == 0; weights with |w| x 64 > 448 are refused at load time. */
  int32_t llm_precision;
} fv_model_desc;

typedef struct fv_tensor_desc {
  const char* name;   /* canonical checkpoint key, e.g. "model.layers.0.self_attn.q_proj.weight" */
  const void* data;   /* contiguous; HOST pointer unless device != 0 */
  int32_t dtype;      /* FV_F32 or FV_BF16 */
  int32_t ndim;
  int64_t shape[4];
  int32_t device;     /* != 0: data is a pointer into the handle's device memory space (copied device-to-device) */
  int32_t reserved;
} fv_tensor_desc;

/* fv_load_weights_cb: called once per tensor the packer needs, in packing order; fills *out (name may stay NULL) and
 * returns 0, or returns non-zero when the checkpoint has no such key.  out->data must stay valid until the next call of
 * the provider (or the end of fv_load_weights_cb): the host side can materialise one tensor at a time (a 7B checkpoint
 * never exists as one 30 GB fp32 dict). */
typedef int (*fv_tensor_provider)(void* user, const char* name, fv_tensor_desc* out);

/* opaque RCCL unique id (ncclUniqueId): made by rank 0 (fv_comm_unique_id), carried to the other ranks by the host side */
typedef struct fv_rccl_id { char internal[128]; } fv_rccl_id;

typedef struct fv_adamw_hparams {
  float lr, beta1, beta2, eps, weight_decay;
  float max_grad_norm; /* <= 0 : no clipping */
  float grad_scale;    /* multiplied into grads before use (1/world_size after a sum all-reduce) */
} fv_adamw_hparams;

/* ---- lifecycle -------------------------------------------------------------------------------------------- */
/* replaces FastVLMBackbone.__init__ / _load_model (model/fastvlm_adapter.py:90-201): create the engine ...
 * The handle owns its weights, the RoPE table, a few KB of counters and ~100 MB of scratch for the few-row launch forms of the tower (fused-ConvFFN
 * hidden ranges, K ranges of the last stages' GEMMs: one to four observations); everything batch-sized is the caller's (fv_workspace_bytes). */
int fv_create(const fv_model_desc* desc, int device, fv_handle** out);
/* ... and pack/fold the frozen weights (BN folding, gate/up interleave, qkv concat, bf16) into library memory. */
int fv_load_weights(fv_handle* h, const fv_tensor_desc* tensors, int n);
/* the same packing with the tensors pulled one at a time through `provider` (streaming load; bf16 sources, on the host
 * or on the device, reach the packed layouts without an fp32 round trip). */
int fv_load_weights_cb(fv_handle* h, fv_tensor_provider provider, void* user);
void fv_destroy(fv_handle* h);
/* last error of a call made on h (per handle); h == NULL: last error raised on the calling thread by fv_create or by a
 * handle-less fv_op_* entry point */
const char* fv_last_error(fv_handle* h);
const char* fv_version(void);

/* bytes of caller-owned scratch needed for batch B, T text tokens (+ image tokens when splice != 0) */
int fv_workspace_bytes(fv_handle* h, int B, int T, int splice, size_t* out_bytes);
int fv_bind_workspace(fv_handle* h, void* ws, size_t bytes);

/* ---- frozen backbone ---------------------------------------------------------------------------------------- */
/* replaces FastVLMBackbone._prepare_images_tensor -> _resize_image -> resize_with_pad
 * (model/fastvlm_adapter.py:36-55,444-461,479-488): img (B,C,Hin,Win) NCHW f32|u8 (C in {1,3,4}) -> pix (B,S,S,4) bf16
 * NHWC (4th channel 0).  resize_with_padding=0 stretches instead (fastvlm_adapter.py:459-460). */
int fv_preprocess(fv_handle* h, const void* img, int dtype, int B, int C, int Hin, int Win, float pad_value,
                  int resize_with_padding, void* pix_out, fv_stream s);
/* fv_preprocess followed by FastVLMBackbone._maybe_normalize_imagenet (model/fastvlm_adapter.py:463-477; `normalize_imagenet=True`, off by default):
 * (x - mean[c]) / std[c] per channel on the letterboxed fp32 values (pad pixels included, as the reference normalises after padding), one bf16 rounding
 * at the end.  range_heuristic != 0 = the torchvision branch (:471-477): if the maximum of the whole letterboxed batch exceeds 1.5 the values are divided
 * by 255 first -- decided on the device from a maximum pass over the same arithmetic (no host synchronisation); 0 = the branch without torchvision
 * (:466-470).  mean / std: 3 floats each in HOST memory. */
int fv_preprocess_normalized(fv_handle* h, const void* img, int dtype, int B, int C, int Hin, int Win, float pad_value, int resize_with_padding,
                             const float* mean3, const float* std3, int range_heuristic, void* pix_out, fv_stream s);
/* ---- on-device image augmentation (an extension of this build; the reference has none) ---------------------------
 * One row per image.  Geometry: the crop window (x0, y0, cw, ch), in continuous SOURCE pixel coordinates, is a view into the real image; the
 * letterbox geometry (resized size, padding) is still that of the full Hin x Win, so the padding never moves.  Output pixel dx of the image region
 * samples sx = max((dx + 0.5) * (cw / rw) - 0.5 + x0, 0), i0 = clamp((int)sx, 0, Win - 1), i1 = min(i0 + 1, Win - 1), w = sx - i0 (rows alike):
 * crop + resize + letterbox is ONE bilinear sample.  Taps outside the window but inside the image read real neighbours, taps outside the image
 * replicate the edge; a non-finite coordinate samples index 0; no row content reads out of range.  Colour (image-region pixels only, on the
 * interpolated fp32 RGB; a gray source's repeated value): v' = clamp(M v + o, 0, value_max), one bf16 rounding at the end; colour == 0 skips the
 * stage, the clamp included.  The identity row (0, 0, Win, Hin, colour 0) gives fv_preprocess's output bit for bit. */
typedef struct fv_augment_sample {
  float x0, y0, cw, ch;
  float m[9], o[3];   /* row-major M, offset */
  int32_t colour;
  int32_t pad[3];     /* 80 bytes */
} fv_augment_sample;
/* ranges (lo, hi) the table is drawn from; HOST memory, 40 bytes.  crop_area: fraction of the image's area; crop_ratio: the window's aspect RELATIVE to
 * the image's own (1, 1 keeps it), drawn log-uniformly; brightness / contrast / saturation: factors, 1 = unchanged */
typedef struct fv_augment_config {
  float crop_area[2], crop_ratio[2], brightness[2], contrast[2], saturation[2];
} fv_augment_config;
/* Draw table_dev[0 .. B) on the device.  Sample b uses two Philox4x32-10 blocks: counter (ctr lo, ctr hi, offset lo, offset hi) with
 * ctr = 2 (sample_base + b) + {0, 1}, key = seed, u_k = (r_k >> 8) 2^-24 (the head's dropout convention): the stream belongs to the GLOBAL sample
 * index, not to the position in the launch.  a = lerp(area, u0), rho = exp(lerp(ln ratio_lo, ln ratio_hi, u1)), cw = clamp(Win sqrt(a rho), 1, Win),
 * ch = clamp(Hin sqrt(a / rho), 1, Hin), x0 = u2 (Win - cw), y0 = u3 (Hin - ch); b, c, s = lerp of the three colour ranges at u4, u5, u6 (u7 reserved);
 * M = b c (s I + (1 - s) 1 w^T), o = (1 - c) b mu 1 with w = (0.299, 0.587, 0.114) and mu the gray mean of the whole source image: brightness ->
 * contrast -> saturation in this fixed order with ONE clamp at the end (torchvision's ColorJitter permutes the order and clamps in between).
 * colour = 0 when all three ranges are (1, 1).  The means: one block per sample, u8 in exact integer sums, f32 in a fixed-order tree, no atomics --
 * the same bits for a given shape every time; skipped (img may be NULL) when contrast is (1, 1).  FV_ERR_ARG before anything is enqueued for null
 * pointers, lo > hi, non-positive area or ratio, negative factors.  No allocation, no host read. */
int fv_augment_draw(fv_handle* h, const fv_augment_config* cfg, const void* img, int dtype, int B, int C, int Hin, int Win,
                    uint64_t seed, uint64_t offset, uint64_t sample_base, fv_augment_sample* table_dev, fv_stream s);
/* fv_preprocess sampling through table_dev (B rows, device memory).  value_max: 255 for u8 sources, 1 for f32 sources in 0..1; <= 0 is FV_ERR_ARG. */
int fv_preprocess_augmented(fv_handle* h, const void* img, int dtype, int B, int C, int Hin, int Win, float pad_value, int resize_with_padding,
                            const fv_augment_sample* table_dev, float value_max, void* pix_out, fv_stream s);
/* replaces the vision tower + mm_projector inside LlavaQwen2ForCausalLM.forward (call site fastvlm_adapter.py:533):
 * pix (B,S,S,4) bf16 -> img_tokens (B, (S/64)^2, llm_hidden) f32.  tower_out (B,(S/64)^2,tower_out_dim) bf16 may be
 * NULL.
 * Kernel forms follow a launch's own tile count: at B <= 2 the fused ConvFFN runs in hidden ranges and the last stages' GEMMs in K ranges (another fp32
 * summation order: <= 1 bf16 step per output), at B <= 4 the depthwise march in row segments (bit-identical to the uncut march); B >= 4 gives an image the
 * same tokens whatever its neighbours.  The same holds for the decoder (fv_llm_forward_pooled: K ranges for <= 256 rows and for ragged row counts <= 1024);
 * the fv_train_* entry points never take these forms. */
int fv_vision_forward(fv_handle* h, const void* pix, int B, void* img_tokens, void* tower_out, fv_stream s);
/* on != 0: the tower keeps the large-batch kernel forms at every batch size (no hidden ranges of the fused ConvFFN, no K ranges in its last stages): an
 * image evaluated alone then gets the tokens it gets inside a batch, bit for bit (measured), at ~0.9 ms per step of a one-observation control loop (4.75 instead of 3.83 ms).
 * Off by default (the host side switches it with FASTVLA_BATCH_INVARIANT=1).  The row-segmented depthwise march is bit-identical and stays on. */
int fv_set_batch_invariant(fv_handle* h, int on);
/* Prompt reuse.  In literal mode (fv_llm_forward_pooled with Ni == 0) the decoder never sees the image: pooled (B, H) is a function of (ids, lens, B, T,
 * pool_mode) and the decoder's weights alone, and a control loop sends the same task string for a whole episode.  The handle keeps ONE slot in device memory
 * (sized at fv_create for max_batch x max_text_tokens): the key of the last literal call and its pooled rows.  Every literal call starts with a one-block
 * probe that compares its key with the slot ON THE DEVICE and ends with a commit launch; on a hit every decoder kernel of the call returns at once and the
 * commit copies the kept rows out, on a miss the decoder runs as ever and the commit stores key and rows.  No host read, no allocation, no synchronisation:
 * the call stays capturable, and a captured graph decides anew on every replay.  A hit returns the bits a recomputation would give.
 *   - compared: B, T, pool_mode, lens[0 .. B), and of every row its first max(min(lens[b], T), 1) ids -- ids past lens[b] cannot reach pooled (causal
 *     attention with keys >= lens[b] masked, row-wise kernels everywhere else, pooling over rows < max(lens[b], 1)).
 *   - invalidated (stream-ordered clear of the slot where the writer takes a stream, and a forced miss of the next call) by everything else pooled depends
 *     on: fv_load_weights / fv_load_weights_cb, fv_train_commit (decoder and tower), fv_train_lora_commit, fv_train_lora_merge,
 *     fv_train_lora_init_magnitude, fv_train_set_options, fv_train_set_forward_f16, fv_set_batch_invariant, fv_set_prompt_reuse.  llm_precision is fixed at
 *     fv_create; the few-row kernel forms follow B and T, which are part of the key.
 *   - never used by the spliced call (Ni > 0), fv_llm_forward_pooled_prefixed, any fv_train_* entry point, or a call whose B x T the slot cannot hold.
 *   - ONE handle serves ONE stream at a time (as its workspace already demands): the slot is read and written in stream order.
 * On by default; on == 0 switches it off (the host side does so for FASTVLA_PROMPT_REUSE=0).  While fv_profile is on, fv_profile_read leaves the flops and
 * bytes of a hit call's skipped launches out (their time and launch count stay) and does not list them among the GEMM shapes. */
int fv_set_prompt_reuse(fv_handle* h, int on);
/* Literal calls that used the slot, and how many of them hit, since fv_create (device counters; synchronises the device). */
int fv_prompt_reuse_stats(fv_handle* h, uint64_t* calls_out, uint64_t* hits_out);
/* fv_preprocess + fv_vision_forward in one (the on-device input pipeline): the stem kernel samples the SOURCE images
 * (B,C,Hin,Win) f32 | u8 through resize_with_pad's arithmetic itself (model/fastvlm_adapter.py:36-55,479-488 then :533), so the letterboxed
 * (B,S,S,4) frame is never written or read.  Same tokens as the two-call form, bit for bit.  Needs the fused stem (first stage width 96). */
int fv_vision_forward_images(fv_handle* h, const void* img, int dtype, int B, int C, int Hin, int Win, float pad_value, int resize_with_padding,
                             void* img_tokens, void* tower_out, fv_stream s);
/* fv_vision_forward that also copies intermediate activation maps out (parity tests name the failing stage with them):
 * taps[0] <- stem output (B,S/4,S/4,dims[0]), taps[1+i] <- output of stage i (B, S/(4<<i), S/(4<<i), dims[i]), bf16 NHWC
 * device buffers; NULL entries are skipped; n_taps <= tower_stages + 1.  The mirror of the oracle's `taps=` argument. */
int fv_vision_forward_taps(fv_handle* h, const void* pix, int B, void* img_tokens, void* tower_out, void* const* taps,
                           int n_taps, fv_stream s);
/* Tower UNITS in execution order: unit 0 = the three stem convolutions, then per stage [RepCPE] block ... block [PatchEmbed]
 * (mci.py `network` ModuleList order; 51 units for fastvithd).  fv_vision_unit_info describes unit u's OUTPUT map
 * (kind 0 stem / 1 RepCPE / 2 block / 3 PatchEmbed; side x side x channels, bf16 NHWC) and fails with FV_ERR_ARG past the last
 * unit.  fv_vision_forward_unit_taps is fv_vision_forward that also copies every unit's output to taps[u] (NULL entries
 * skipped): unit u's input is taps[u-1], so a parity test can feed the ORACLE unit the ENGINE's own input and compare one unit
 * at a time (teacher forcing: no error amplification through the 44 blocks).  Same call site as fv_vision_forward
 * (model/fastvlm_adapter.py:533). */
int fv_vision_unit_info(fv_handle* h, int unit, int32_t* kind, int32_t* stage, int32_t* side, int32_t* channels);
int fv_vision_forward_unit_taps(fv_handle* h, const void* pix, int B, void* img_tokens, void* tower_out, void* const* taps,
                                int n_taps, fv_stream s);
/* replaces embed_tokens + L x Qwen2DecoderLayer + final RMSNorm + FastVLMBackbone._pool_hidden
 * (fastvlm_adapter.py:533,551-559,337-359): ids (B,T) int32 right-padded, lens (B) int32,
 * img_tokens NULL (literal reference: text-only sequence) or (B,Ni,H) f32 spliced in front of the text.
 * pool_mode 0 = last_token, 1 = mean_pool.  pooled (B,H) f32. */
int fv_llm_forward_pooled(fv_handle* h, const int32_t* ids, const int32_t* lens, const void* img_tokens, int Ni, int B,
                          int T, int pool_mode, void* pooled, fv_stream s);

/* llm_precision >= 2 runs gate/up and down on fp16 operands.  Weights outside the binary16 range are REFUSED at load time
 * (fv_load_weights* returns FV_ERR_UNSUPPORTED: load with llm_precision = 1); activations are converted with SATURATING casts
 * (an outlier channel of a real checkpoint clamps to +-65504 instead of becoming inf / NaN actions) and every clamped 8-value
 * group is counted.  This reads the counter (0 in a healthy model; non-zero = the fp16 budget does not hold for this
 * checkpoint / input, switch to llm_precision = 1).  A status call: synchronises the device.  Call site whose fp32 arithmetic
 * this guards: model/fastvlm_adapter.py:183-191 (the reference loads fp32), :533. */
int fv_llm_fp16_saturations(fv_handle* h, uint64_t* count_out, int reset);

/* Image-prefix reuse (the call site the reference has is ONE full prefill per env step:
 * lerobot_fastvla/modeling_fastvla.py:119-125 -> model/fastvlm_adapter.py:519-536).  With the image tokens spliced in FRONT of the
 * text under a causal mask, the keys / values of the Ni image positions depend on the image alone:
 *   fv_llm_prefix            runs those positions through the decoder once and writes every layer's un-rotated [k | v] rows to
 *                            kv_out ([llm_layers][B * Ni][2 * kv_heads * head_dim] f32, caller-owned, fv_llm_prefix_bytes);
 *   fv_llm_forward_pooled_prefixed  runs ONLY the T text positions against that cache: the same pooled rows as
 *                            fv_llm_forward_pooled(img_tokens, Ni) up to the summation order of other tile shapes.
 * A caller that keeps kv per image (or per camera frame) skips tower, projector and prefix for a repeated frame or for further
 * prompts on the same image.  llm_precision 1 / 2 and head_dim 64 / 128 only; pool_mode must be 0 (last_token). */
int fv_llm_prefix_bytes(fv_handle* h, int B, int Ni, size_t* out_bytes);
int fv_llm_prefix(fv_handle* h, const void* img_tokens, int Ni, int B, void* kv_out, fv_stream s);
int fv_llm_forward_pooled_prefixed(fv_handle* h, const int32_t* ids, const int32_t* lens, const void* kv, int Ni, int B, int T,
                                   int pool_mode, void* pooled, fv_stream s);

/* ---- action expert (trainable; parameters live in ONE caller-owned flat f32 buffer) --------------------------- */
/* element offsets of the 12 head tensors inside the flat buffer, in state-dict order
 * (state_projection.0.{weight,bias}, state_projection.1.*, fusion.0.*, fusion.1.*, fusion.4.*, action_head.*);
 * offsets[12] = total element count. */
int fv_head_layout(fv_handle* h, int64_t offsets[13]);
int fv_head_saved_bytes(fv_handle* h, int B, size_t* out_bytes);
/* replaces FastVLMWithExpert.forward after the backbone (fastvla/fastvlm_with_expert.py:50-54).
 * training: 0 = inference; 1 = training, Dropout(p) applied with a Philox mask derived from (seed, offset); 2 = training without
 * dropout (p = 0).  Any non-zero value keeps the actions in normalised space when fv_head_set_io_norm folded the dataset
 * statistics in (the loss is computed against normalised targets).  saved = activations for backward. */
int fv_head_forward(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B,
                    int training, float dropout_p, uint64_t seed, uint64_t offset, float* actions, void* saved,
                    fv_stream s);
/* Dataset statistics folded into the head: replaces the STATE / ACTION parts of LeRobot's
 * NormalizerProcessorStep / UnnormalizerProcessorStep around the policy (lerobot_fastvla/processor_fastvla.py:34-48, MEAN_STD per
 * lerobot_fastvla/configuration_fastvla.py:21-27): fv_head_forward then computes LayerNorm((states - state_mean) / (state_std + eps))
 * ... and, when training == 0, returns actions * action_std + action_mean.  HOST vectors of state_dim / action_dim floats; all four
 * NULL switches the folding off.  Training keeps its loss in normalised action space (targets arrive normalised).
 * A configuration call: it synchronises the device before overwriting the handle's ONE statistics vector.  A hipGraph captured
 * over fv_head_forward keeps the on/off state of its capture: re-capture after switching the folding on or off (new VALUES
 * written while it stays on are picked up by replays, the vector's address does not change). */
int fv_head_set_io_norm(fv_handle* h, const float* state_mean, const float* state_std, const float* action_mean,
                        const float* action_std, float eps);
/* replaces F.mse_loss + autograd backward of the head (fastvla/modeling_fastvla.py:56,
 * lerobot_fastvla/modeling_fastvla.py:132; trainer.py:175): writes loss (1 f32, device) and ALL 12 grads into
 * flat_grads (overwritten, not accumulated). */
int fv_head_mse_backward(fv_handle* h, const float* flat_params, const float* actions, const float* targets, int B,
                         float dropout_p, const void* saved, float* loss, float* flat_grads, fv_stream s);
/* ---- action chunks and the loss of the fused backward.  The head's output width stays fv_model_desc.action_dim = K * A: a chunk of K future steps of A
 * action dimensions each, row-major (B, K, A).  The loss below is what fv_head_mse_backward and every fv_train_*_forward_backward evaluate (one place:
 * the head backward), so all of them take the spec and the mask from the handle.  With d = actions - targets, n = B * K * A and w = 0 where pad[b][k] else 1:
 *     loss = sum w rho(d) / n          dL/dactions = loss_scale * w * rho'(d) / n       (rho as torch: mse d^2; l1 |d|, sign(0) = 0;
 *     smooth_l1 0.5 d^2 / beta for |d| < beta, else |d| - 0.5 beta)
 * The denominator is ALL n elements, padded ones included (LeRobot's `(loss * ~pad).mean()`): micro-batches and data-parallel ranks with different pad
 * counts then still average exactly.  A padded element gives exactly 0 to the loss, the metrics and the gradient whatever its target holds (NaN, inf).
 * kind MSE with no mask (and no weights: fv_head_set_loss_weights) launches the single-block MSE kernel it always did, for any K; everything else a many-block kernel with fixed-order partials
 * and a single-block fold (no float atomics: two runs agree bit for bit). */
#define FV_LOSS_MSE 0
#define FV_LOSS_L1 1
#define FV_LOSS_SMOOTH_L1 2
typedef struct fv_head_loss_spec {
  int32_t kind;    /* FV_LOSS_* */
  float beta;      /* smooth-L1 threshold, > 0 (read for FV_LOSS_SMOOTH_L1 only) */
  int32_t chunk;   /* K >= 1, action_dim % K == 0 */
} fv_head_loss_spec;
/* NULL = {FV_LOSS_MSE, -, 1}.  FV_ERR_ARG for an unknown kind, a smooth-L1 beta that is not a positive finite number, K < 1 or K not dividing
 * action_dim; nothing is enqueued.  A configuration call without device work.  A hipGraph captured over a loss evaluation keeps the spec AND the
 * mask pointer of its capture: re-capture after either setter (new mask VALUES written to the same address are picked up by replays). */
int fv_head_set_loss(fv_handle* h, const fv_head_loss_spec* spec);
/* pad_dev: DEVICE (B, K) bytes, 1 = padded step; NULL = none.  Read by every later loss evaluation on the handle until replaced; the caller keeps it
 * alive (and sized for the B of those calls). */
int fv_head_set_loss_mask(fv_handle* h, const uint8_t* pad_dev);
/* *dev = 2 handle-owned device floats written by the chunked loss kernel (not by the plain MSE path): { sum over valid elements of d^2 / n,
 * valid steps / (B * K) }.  They head a 16-byte aligned slot of 4 floats of their own (the other two stay 0): a 4-float copy is in bounds.
 * (A binned head -- fv_head_set_bins, below -- writes the slot with every loss evaluation and uses the third float for its accuracy.) */
int fv_head_loss_metrics(fv_handle* h, const float** dev);
/* Per-dimension and per-step weights of the loss above (gripper against arm, near against far steps).  dim_w: HOST, A = action_dim / chunk floats; step_w:
 * HOST, K = chunk floats; either may be NULL, meaning ones; both NULL switches weighting off.  With om = dim_w[a] * step_w[k]:
 *     loss = sum_valid om rho(d) / n          dL/dactions = loss_scale * om * rho'(d) / n          (n stays ALL B K A elements)
 * An element with om == 0 is SELECTED away exactly like a padded one: 0 to the loss, the gradient and the masked MSE whatever its target holds (NaN, inf).
 * The two metrics stay UNWEIGHTED (masked MSE; valid steps / (B K), which looks at pads only), so runs with different weights remain comparable.
 * With weights on EVERY kind, plain MSE without a mask included, runs the many-block kernel's weighted instance (and writes the metrics); with weights off
 * every loss evaluation launches what it launched before.  Weights that are all exactly 1 give the bits of the unweighted many-block kernel.
 * Values must be finite and >= 0: FV_ERR_ARG otherwise, with no state changed.  A configuration call: it synchronises the device before it overwrites
 * the handle's ONE weight vector.  A later fv_head_set_loss that CHANGES chunk drops the weights (their sizes no longer fit): set them again after it.
 * A hipGraph captured over a loss evaluation keeps the on/off state of its capture. */
int fv_head_set_loss_weights(fv_handle* h, const float* dim_w, const float* step_w);
/* out_dev[a] (A = action_dim / chunk DEVICE floats) = mean |actions - targets| over the non-padded steps of action dimension a, in the (normalised) space
 * the loss lives in; 0 for a dimension without a valid step.  actions, targets: (B, K, A) device f32.  Uses the handle's current chunk and mask, never the
 * weights.  One block per dimension, fixed-order sums (no float atomics).  On demand: no train step calls it. */
int fv_head_loss_per_dim(fv_handle* h, const float* actions, const float* targets, int B, float* out_dev, fv_stream s);
/* ---- binned action head ("discretised actions", OpenVLA / RT-2; normalised action space).  action_head becomes Linear(fusion_dim, action_dim * bins): the
 * logits are (B, K, A, bins) row-major and the `bins` logits of one action element are a GROUP.  The 12 tensors, their names and order stay; action_dim stays
 * the ACTION width K * A everywhere a caller sees it; fv_head_layout, fv_head_saved_bytes, the workspace and the training layouts follow the taller tensor.
 * Element e of a row has the range [lo, hi] = entry e % n_range of the two host vectors.  w = (hi - lo) / bins (formed in double, rounded to fp32 once); bin j
 * covers [lo + j w, lo + (j + 1) w) and has the centre c_j = lo + (j + 1/2) w; a target a is clamped to [lo, hi] and falls into bin min(bins - 1, floor((a - lo) / w)).
 * Target distribution q of a group: sigma == 0 one-hot at the target's bin; sigma > 0 (HL-Gauss, sigma in units of w, S = sigma w) the Gaussian around the
 * clamped target integrated over the bins and renormalised to the range,
 *     q_j = [Phi((e_{j+1} - a) / S) - Phi((e_j - a) / S)] / [Phi((hi - a) / S) - Phi((lo - a) / S)],  e_j = lo + j w (the last edge is hi itself),
 * evaluated in double inside the kernel and rounded to fp32 once.  With p = softmax(z), n = B K A (ALL elements) and om as fv_head_set_loss_weights:
 *     loss = sum_valid om (-sum_j q_j log p_j) / n          dL/dz_j = loss_scale om (p_j - q_j) / n
 * A padded step (fv_head_set_loss_mask) or an element with om == 0 is SELECTED away: exactly 0 to the loss, the metrics and all `bins` gradient elements,
 * its target never read.  Decode: FV_BINS_DECODE_ARGMAX the centre of the most likely bin (ties to the lowest index), FV_BINS_DECODE_MEAN sum_j p_j c_j.
 * In bins mode
 *   fv_head_forward writes the logits into `saved` (fv_head_bins_logits) and the DECODED (B, action_dim) chunk to `actions`: normalised when training != 0,
 *     with the folded action statistics of fv_head_set_io_norm applied behind the decode otherwise;
 *   fv_head_mse_backward and every fv_train_*_forward_backward evaluate the loss above from the saved logits and `targets` (continuous, normalised; `actions`
 *     is not read) -- FV_ERR_STATE unless the configured loss kind is the default FV_LOSS_MSE (the kind has no meaning here; chunk, mask and weights apply);
 *   fv_head_backward (a caller's grad_actions) is refused with FV_ERR_STATE: the decode is not differentiated, the head trains through its own loss;
 *   fv_head_loss_metrics' 4-float slot is written by every loss evaluation: { sum_valid (decoded - target)^2 / n, valid steps / (B K), the fraction of the
 *     valid elements whose most likely bin is the target's, 0 } -- unweighted, valid looks at pads only, an om == 0 element adds no error and is no hit.
 * One wave per group, the logits read once, fixed-order sums (no float atomics: two runs agree bit for bit). */
#define FV_BINS_DECODE_ARGMAX 0
#define FV_BINS_DECODE_MEAN 1
#define FV_HEAD_BINS_MAX 1024
#define FV_HEAD_BINS_MAX_WIDTH 32768   /* action_dim * bins: the head's linear kernels put one output per block row, a wide-output GEMM is not built */
typedef struct fv_head_bins_spec {
  int32_t bins;      /* 2 .. FV_HEAD_BINS_MAX */
  int32_t decode;    /* FV_BINS_DECODE_* */
  float sigma;       /* >= 0, finite; 0 = one-hot targets */
  int32_t n_range;   /* entries of lo_host / hi_host: >= 1 and a divisor of action_dim (1: one range for all; A: one per action dimension) */
} fv_head_bins_spec;
/* NULL spec switches the mode off: the handle is the regression head again, bit for bit.  Allowed only BEFORE fv_bind_workspace and before any
 * fv_train_*_begin (FV_ERR_STATE afterwards: sizes depend on the mode), and not while flow mode is on (FV_ERR_STATE; fv_head_set_flow answers the same while
 * bins are on).  FV_ERR_ARG, changing nothing, for bins outside 2 .. 1024, an unknown decode, a negative or non-finite sigma, n_range < 1 or not dividing
 * action_dim, a null, non-finite or unordered (lo >= hi) range, action_dim * bins > FV_HEAD_BINS_MAX_WIDTH.  A configuration call: it uploads the ranges. */
int fv_head_set_bins(fv_handle* h, const fv_head_bins_spec* spec, const float* lo_host, const float* hi_host);
/* *logits_dev = the (B, action_dim, bins) logits a bins-mode fv_head_forward(B) wrote into `saved`.  FV_ERR_STATE when bins mode is off. */
int fv_head_bins_logits(fv_handle* h, const void* saved, int B, const float** logits_dev);
/* probs_dev (B, action_dim, bins) DEVICE f32 <- softmax of every group of those logits (the decode kernel's own max-subtracted softmax), one launch on s.
 * FV_ERR_STATE when bins mode is off. */
int fv_head_bins_probs(fv_handle* h, const void* saved, int B, float* probs_dev, fv_stream s);
/* ---- flow-matching action head (pi0 / SmolVLA convention, everything in normalised action space).  With eps ~ N(0, I), a the target chunk and t in [0, 1]:
 *     x_t = t eps + (1 - t) a        u = eps - a        sampling: x_1 = eps, x <- x + dt v for N steps of dt = -1 / N down to t = 0
 * The velocity network v(x_t, t | observation) is the SAME expert with two more input blocks on fusion.0:
 *     cat = [ pooled (llm_hidden) | state branch (hidden_dim) | x_t (action_dim) | phi(t) (time_dim) ]
 *     phi(t) = [ sin(2 pi t / p_j) | cos(2 pi t / p_j) ], j < time_dim / 2, p_j geometric from min_period to max_period
 * so the 12 tensors, their names and order and fv_head_layout's 13 offsets stay; only fusion.0.weight's column count (and with it the offsets behind it,
 * fv_head_saved_bytes, the workspace and the training layouts) grows.  The action width is the handle's action_dim (= K * A).
 * time_dist: 0 draws t ~ U[0, 1), 1 logit-normal t = sigmoid(dist_a + dist_b n), n ~ N(0, 1). */
typedef struct fv_head_flow_spec {
  int32_t time_dim;                 /* E: even, >= 2 */
  float min_period, max_period;     /* finite, 0 < min_period < max_period (pi0: 4e-3, 4.0) */
  int32_t time_dist;                /* 0 uniform, 1 logit-normal */
  float dist_a, dist_b;             /* finite (read for time_dist 1 only) */
} fv_head_flow_spec;
/* NULL switches flow mode off: the handle is then the regression head it was, bit for bit.  Allowed only BEFORE fv_bind_workspace and before any
 * fv_train_*_begin (FV_ERR_STATE afterwards: sizes depend on the mode).  FV_ERR_ARG, changing nothing, for an odd or non-positive time_dim, non-positive,
 * unordered or non-finite periods, an unknown time_dist, a non-finite dist_a / dist_b.  A configuration call: it uploads time_dim / 2 frequencies. */
int fv_head_set_flow(fv_handle* h, const fv_head_flow_spec* spec);
/* Training's noising step, ONE launch: per row b a time t and per element a normal eps (Box-Muller on Philox4x32-10; the key differs from the dropout
 * stream's, so the same (seed, offset) may serve both; the counter is a function of (row, element, offset) only: row b draws the same values whatever B is).
 * Writes x_t and phi(t) straight into their columns of `saved` (fv_head_saved_bytes(B) bytes, the buffer the following fv_head_forward is given) and
 * u = eps - targets into u_out (B, action_dim).  targets: (B, action_dim) device f32, normalised.  noise (B, action_dim) / t (B): device f32 that REPLACE the
 * draws, either may be NULL.  In flow mode fv_head_forward leaves those columns alone and reads them: fv_head_flow_prepare ON THE SAME `saved` MUST COME FIRST;
 * its output is the predicted velocity, and fv_head_mse_backward(actions = v, targets = u) evaluates the configured loss (kind, mask, weights) on velocities.
 * The fv_train_*_forward_backward routes do the same internally from their own (seed, offset) and targets.
 * (seed, offset) TRAVEL AS KERNEL ARGUMENTS: a hipGraph captured over this call bakes them in and replays the same draws -- inside a captured step hand
 * in noise and t buffers and refresh those.  Asynchronous on s, allocates nothing.  FV_ERR_STATE when flow mode is off, FV_ERR_ARG for a null targets /
 * saved / u_out or B < 1; nothing is enqueued then. */
int fv_head_flow_prepare(fv_handle* h, const float* targets, int B, uint64_t seed, uint64_t offset, const float* noise, const float* t, void* saved,
                         float* u_out, fv_stream s);
/* Several noise draws per observation in ONE training step: draws = S, 1 .. FV_FLOW_DRAWS_MAX (1, the default, is the handle as it was, bit for bit;
 * fv_head_set_flow(NULL) returns it to 1).  The step then computes the mean loss and the mean gradient of S single-draw steps for one backbone pass.
 * DRAW OFFSET: draw s of row b is exactly what a single-draw call draws for row b at offset + (s << 56) -- the key, the counter (group, row, offset) and
 * the Box-Muller are unchanged -- so draw 0 is the single draw and row b's draws depend neither on B nor on S.  Bits 56 .. 59 of `offset` therefore belong
 * to the draw index: with S > 1 an offset that has one of them set is refused (FV_ERR_ARG, nothing enqueued) by fv_head_flow_prepare and the train routes.
 * HEAD ROWS are draw-major, r = s B + b.  In every training-side head call B counts OBSERVATIONS (B <= max_batch as ever): targets, pad mask (B, K), pooled
 * and states keep B rows and apply to every draw of their observation; noise, t, u_out, the predicted velocity (`actions` of fv_head_forward with
 * training != 0, of fv_head_mse_backward and fv_head_loss_per_dim) and grad_actions have S B rows; rows 0 .. B - 1 are the single-draw call's rows.
 * fv_head_saved_bytes, the workspace and the training workspace are sized for S B head rows.  The loss divides by all S B K A elements; the 12 head
 * gradients are sums over all S B rows; d_pooled and the state branch's gradient are summed over the draws in ascending s (fixed order, no atomics).
 * The state branch runs once per observation.  The train routes keep every draw's prediction in their workspace and write draw 0's rows to the caller's
 * (B, action_dim) `actions`.  Inference (fv_head_forward with training == 0) and the samplers ignore the setting.
 * Allowed only in flow mode, BEFORE fv_bind_workspace and before any fv_train_*_begin (FV_ERR_STATE otherwise); FV_ERR_ARG, changing nothing, outside 1 .. 16. */
#define FV_FLOW_DRAWS_MAX 16
int fv_head_set_flow_draws(fv_handle* h, int draws);
/* The distribution of the training time, beyond fv_head_set_flow's two: every drawn t becomes t = t_lo + (t_hi - t_lo) tau with tau = F^-1(u), u taken from the
 * ONE 24-bit uniform the noising kernel already draws (k = x >> 8 of the group-0 Philox block; u = k 2^-24 in double).  Nothing is rejected and nothing loops on
 * the random stream: a row's draws still depend on (seed, offset, row) alone, and eps, u_out, the prefix delay and the dropout stream do not move.
 *     dist 0 uniform: tau = u.     dist 2 Beta(a, b): tau = I^-1_u(a, b), the inverse regularised incomplete beta function, evaluated in double.
 *     dist 1 logit-normal: tau = sigmoid(a + b n) with fv_head_set_flow's Box-Muller n and its bits; stratified: n = Phi^-1(u), and u = 0 gives tau = 0.
 *     stratify (with S = fv_head_set_flow_draws > 1): draw s takes the s-th of S equal-probability strata, u = (s + k 2^-24) / S.  With S = 1 it does nothing.
 * t is formed in double and rounded to fp32 once.  pi0 / SmolVLA: {2, 1.5, 1.0, 0.001, 1.0, 0}.  Explicit t buffers still replace every draw.
 * NULL returns the handle to what fv_head_set_flow's own time_dist / dist_a / dist_b say, bit for bit; fv_head_set_flow (NULL or a spec) resets it.  A handle
 * that never calls this launches what it always launched.  No size depends on it: allowed at any time in flow mode (FV_ERR_STATE when flow mode is off).
 * FV_ERR_ARG, changing nothing, for an unknown dist, a non-finite field, a Beta a or b outside [0.25, 32], a range that is not 0 <= t_lo < t_hi <= 1,
 * stratify not 0 or 1.  A hipGraph captured over a noising launch keeps the setting of its capture. */
typedef struct fv_head_flow_time_spec {
  int32_t dist;       /* 0 uniform, 1 logit-normal (a + b n), 2 Beta(alpha = a, beta = b) */
  float a, b;
  float t_lo, t_hi;   /* t = t_lo + (t_hi - t_lo) * tau, 0 <= t_lo < t_hi <= 1 */
  int32_t stratify;   /* 0 | 1: draw s of S takes the s-th of S equal-probability strata */
} fv_head_flow_time_spec;
int fv_head_set_flow_time(fv_handle* h, const fv_head_flow_time_spec* spec);
/* The velocity error as a function of t: out_dev (n_buckets, 2) DEVICE floats, per bucket { sum over non-padded elements of (actions - targets)^2, the number
 * of those elements }; an empty bucket reads (0, 0).  actions = v, targets = u: (R, action_dim) device f32, t: (R) device f32, R = B head rows (S B with
 * fv_head_set_flow_draws, as fv_head_loss_per_dim).  Row r falls into bucket min(n_buckets - 1, (int)(t n_buckets)), t clamped to [0, 1].  Uses the handle's
 * chunk and (B, K) mask, never the loss kind or the weights.  One block per bucket, rows in ascending order, fixed-order sums, no atomics: two calls give the
 * same bits.  Asynchronous on s, allocates nothing.  FV_ERR_STATE when flow mode is off, FV_ERR_ARG for a null pointer, B < 1 or n_buckets outside 1 .. 64;
 * nothing is enqueued then. */
#define FV_LOSS_TIME_BUCKETS_MAX 64
int fv_head_loss_per_time(fv_handle* h, const float* actions, const float* targets, const float* t, int B, int n_buckets, float* out_dev, fv_stream s);
/* Inference: n_steps Euler steps from x_1 = noise (B, action_dim; NULL: the normals fv_head_flow_prepare would draw for (seed, offset)) to actions
 * (B, action_dim), un-normalised on the last step when fv_head_set_io_norm is on.  The state branch and the part of fusion.0 that does not depend on t,
 * c = W[:, :llm_hidden + hidden_dim] . [pooled | s] + b, are computed ONCE per call; every step then runs three launches that touch only fusion.0's last
 * action_dim + time_dim columns, fusion.4 and action_head.  No dropout, no atomics, no host synchronisation, no allocation: the rows live in the bound
 * workspace (fv_workspace_bytes grows with the mode), every reduction has a fixed order, two calls give the same bits.  n_steps travels as host state of the
 * call: a captured graph keeps the step count and, with noise == NULL, the (seed, offset) of its capture.
 * FV_ERR_STATE when flow mode is off or no workspace is bound, FV_ERR_ARG for n_steps < 1, B outside 1 .. max_batch or a null pointer; nothing is enqueued. */
int fv_head_flow_sample(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                        uint64_t seed, uint64_t offset, float* actions, fv_stream s);
/* ---- real-time chunking (Black, Galliker, Levine 2025): the new chunk is sampled GUIDED by the not-yet-executed rest of the previous one.  Per Euler step,
 * with a^ = x - t v(x, t) the denoised estimate, Y the target rows and w[k] >= 0 the weight of step k (broadcast over its action_dim / chunk dimensions):
 *     omega = w (Y - a^)      g = omega - t J^T omega, J = dv / dx      k_i = beta at t = 1, else min(beta, ((1 - t)^2 + t^2) / ((1 - t) t))
 *     v' = v - k_i g          x <- x + dt v'
 * (the paper's tau is 1 - t and its velocity has the other sign).  An element with w == 0 is SELECTED to omega = 0 whatever Y holds.
 * Configuration call: uploads `chunk` HOST floats (finite, >= 0; fastvla_hip.rtc.prefix_weights builds the paper's schedule) and keeps beta =
 * max_guidance_weight (finite, > 0).  step_weights_host == NULL switches guidance off.  FV_ERR_STATE when flow mode is off.  FV_ERR_ARG, changing nothing, for
 * chunk < 1, action_dim % chunk != 0, a negative or non-finite weight, a non-finite or non-positive max_guidance_weight.  The guided sampler's rows join the
 * workspace plan with the FIRST call (fv_workspace_bytes grows from then on and stays): that call must come before fv_bind_workspace (FV_ERR_STATE afterwards);
 * later calls with the same chunk may change weights and beta at any time (they synchronise the device).  A handle that never calls it reports the
 * fv_workspace_bytes it always did and launches what it always launched. */
int fv_head_set_flow_guidance(fv_handle* h, int chunk, const float* step_weights_host, float max_guidance_weight);
/* fv_head_flow_sample with guidance.  prev: (B, action_dim) device f32, the previous chunk in NORMALISED space; Y[b][k] = prev[b][k + shift] for
 * k + shift < chunk (the shift happens inside the kernel), steps with k + shift >= chunk count as weight 0.  row_mask: (B) device int32 or NULL (all rows);
 * a row with 0 is unguided.  chunk_out: (B, action_dim) device f32 or NULL, the final normalised x_0 (before the folded un-normalisation): the next call's
 * `prev`.  Everything else as fv_head_flow_sample.  A row whose row_mask is 0 or whose weights are all 0 comes out as fv_head_flow_sample's row BIT FOR BIT.
 * Conditioning once, then 8 launches per step: the unguided forward (keeping the fusion.4 pre-activation and v), omega, three transposed products that read
 * the row-major weights as stored (action_head over the steps up to the last non-zero weight only, fusion.4, the x columns of fusion.0) with a LayerNorm
 * backward between the last two, and the update.  No atomics, no host synchronisation, no allocation; every reduction has a fixed order: two calls give the
 * same bits.  shift, n_steps, the step times t_i and the guidance weights k_i are HOST STATE of the call that travels as kernel arguments: a captured graph
 * bakes them in (and, with noise == NULL, the (seed, offset) of its capture).
 * Refused before anything is enqueued: FV_ERR_STATE when flow mode is off, guidance is not configured or no workspace is bound; FV_ERR_ARG for a null
 * flat_params / pooled / states / prev / actions, shift outside 0 .. chunk, n_steps < 1, B outside 1 .. max_batch. */
int fv_head_flow_sample_guided(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                               uint64_t seed, uint64_t offset, const float* prev, int shift, const int32_t* row_mask, float* actions, float* chunk_out,
                               fv_stream s);
/* ---- action-prefix conditioning (Black, Ren, Equi, Levine 2025, "Training-time action conditioning for efficient real-time chunking"): the conditioning
 * that guidance approximates at inference time moves into training.  A delay d <= D is drawn per head row; the first d steps of the chunk reach the network
 * CLEAN, only the rest is noised and only the rest trains.  This head has one phi(t) for the whole flattened chunk, so the prefix travels as one more block:
 *     cat = [ pooled | state branch | x_t (action_dim) | phi(t) (time_dim) | m (chunk) ]      m[k] = 1 for k < d, else 0
 *     x_t[k, :] = a[k, :] exactly (a copy) for k < d, as ever for k >= d
 * Only fusion.0.weight grows, by `chunk` columns behind phi; the 12 tensors, their order and fv_head_layout's 13 offsets stay.  A conditioned step is treated
 * by the loss exactly like a padded one (0 to the loss and to every gradient; the divisor stays all S B K A elements); u is written everywhere as ever.
 * fv_head_loss_metrics keeps reporting the pad-only valid fraction; its masked MSE is over the trained elements.
 * chunk = K >= 2 divides action_dim and must be the loss's chunk length (fv_head_set_loss) whenever the fused loss runs (FV_ERR_STATE from the backward
 * otherwise); max_delay = D, 1 <= D <= K - 1; thresholds_host: D + 1 non-decreasing HOST uint32, the cumulative delay distribution in units of 2^-24, the
 * last one 2^24 (fastvla_hip.prefix.delay_thresholds builds it).  NULL thresholds switch the mode off, as fv_head_set_flow(NULL) does: every size and every
 * launch is then the flow head's.  Allowed only in flow mode, BEFORE fv_bind_workspace and before any fv_train_*_begin (FV_ERR_STATE otherwise); FV_ERR_ARG,
 * changing nothing, for invalid input.  fv_head_saved_bytes, the workspace and the training layouts grow by the K mask columns and a (head rows, K) byte mask
 * inside `saved`.
 * THE DELAY of a head row comes from the group-0 Philox block that yields t: t uses words x and y, d is the smallest j with (z >> 8) < thresholds[j] -- an
 * integer compare, no new stream, no new counter: t and eps are the bits a plain flow head draws for the same (seed, offset, row), and draw s of an S-draw
 * step is still the single draw at offset + (s << 56), delay included.  fv_head_flow_prepare keeps its signature and draws the delays in prefix mode;
 * fv_head_flow_prepare_prefix takes them explicitly (device int32, one per head row, clamped to 0 .. D inside the kernel), as noise and t do: the form for
 * tests and captured graphs.  One launch writes x_t, phi(t), m, u and the byte mask.
 * fv_head_flow_sample, fv_head_flow_sample_guided and fv_head_forward with training == 0 work on a prefix-width head with m = 0. */
int fv_head_set_flow_prefix(fv_handle* h, int chunk, int max_delay, const uint32_t* thresholds_host);
int fv_head_flow_prepare_prefix(fv_handle* h, const float* targets, int B, uint64_t seed, uint64_t offset, const float* noise, const float* t,
                                const int32_t* delays, void* saved, float* u_out, fv_stream s);
/* fv_head_flow_sample with the first steps of the chunk pinned.  prev: (B, action_dim) device f32, the previous chunk in NORMALISED space; delays: (B) device
 * int32.  Row b pins its first min(delays[b], D, K - shift) steps to prev[b][k + shift] (the clamp runs inside the kernels: no host synchronisation); they
 * leave in chunk_out ((B, action_dim) or NULL, normalised) as the bits they came in with and in `actions` as fmaf(prev, action_std, action_mean) when
 * fv_head_set_io_norm is on.  A delay of 0 pins nothing.  Whatever prev holds outside the pinned range (NaN, +-inf) is never read.
 * Conditioning once (the mask block's sum of fusion.0 columns joins it), then three launches per step, as fv_head_flow_sample: no guidance, no Jacobian,
 * no atomics, no allocation, every sum in a fixed order: two calls give the same bits.  shift, n_steps and the step times are host state of the call.
 * Refused before anything is enqueued: FV_ERR_STATE when flow mode or prefix mode is off or no workspace is bound; FV_ERR_ARG for a null flat_params /
 * pooled / states / prev / delays / actions, shift outside 0 .. K, n_steps < 1, B outside 1 .. max_batch. */
int fv_head_flow_sample_prefix(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                               uint64_t seed, uint64_t offset, const float* prev, int shift, const int32_t* delays, float* actions, float* chunk_out,
                               fv_stream s);
/* ---- higher-order integrators for all three samplers (fv_head_flow_sample, _prefix, _guided).  Explicit Runge-Kutta schemes whose stage j + 1 depends on
 * stage j only; within a step from t_i to t_i + h, h = -1 / n_steps, with k_j = v(x_j, t_i + c_j h):
 *     x_1 = x0      x_{j+1} = x0 + (a_{j+1} h) k_j      x <- x0 + h sum_j b_j k_j
 *     midpoint  c = 0, 1/2          a = 1/2          b = 0, 1
 *     Heun      c = 0, 1            a = 1            b = 1/2, 1/2
 *     RK4       c = 0, 1/2, 1/2, 1  a = 1/2, 1/2, 1  b = 1/6, 1/3, 1/3, 1/6
 * n_steps keeps meaning STEPS: a call makes n_steps x stages network evaluations, each the Euler step's launches with the x update replaced by a stage
 * update over two more (B, action_dim) rows, the step's start and the running sum.  The stage times 1 - (i + c_j) / n_steps, the products a_j h, the b_j and
 * h are formed on the host in double and rounded once.  The guided sampler evaluates the corrected velocity v' with the STAGE's t and guidance weight; the
 * prefix sampler leaves a pinned element alone at every stage.  Everything the three entry points promise stays: no atomics, no host synchronisation, no
 * allocation, rows never meet, two calls give the same bits, a guided row with omega == 0 is the plain sampler's row of the same solver bit for bit.
 * Configuration call, for all three entry points; their signatures do not change.  FV_ERR_STATE when flow mode is off; FV_ERR_ARG, changing nothing, for an
 * unknown solver.  The two rows join the workspace plan with the FIRST call that names a solver other than Euler (fv_workspace_bytes grows from then on and
 * stays): that call must come before fv_bind_workspace (FV_ERR_STATE afterwards); later calls switch freely among all four.  A handle that never names one
 * reports the fv_workspace_bytes it always did; FV_FLOW_SOLVER_EULER is the scheme with one stage and needs neither row.  fv_head_set_flow(NULL) returns it to Euler. */
#define FV_FLOW_SOLVER_EULER 0
#define FV_FLOW_SOLVER_MIDPOINT 1
#define FV_FLOW_SOLVER_HEUN 2
#define FV_FLOW_SOLVER_RK4 3
int fv_head_set_flow_solver(fv_handle* h, int solver);
/* ---- several samples per observation, one chosen on the device.  A call draws S candidates per observation and returns ONE of them: the one the others
 * agree with (MEDOID: the smallest sum of squared distances to the rest), the one that continues the previous chunk (COHERENT: the backward-coherence
 * criterion of Bidirectional Decoding, Liu et al. 2024), or simply candidate 0 (FIRST).  The mean of the candidates is deliberately not offered: between
 * two modes it is a chunk the policy never learned.
 * Head rows are sample-major, r = s B + b, and candidate s of a call at offset o is EXACTLY the single-sample call at o + (s << 56), as the draws of
 * fv_head_set_flow_draws are: candidate 0 is fv_head_flow_sample's (fv_head_flow_sample_prefix's) output bit for bit.  Bits 56 .. 59 of the offset number the
 * candidates: with S > 1 an offset that has one of them set is refused (FV_ERR_ARG, nothing enqueued).
 * fv_head_set_flow_samples: max_samples 1 .. FV_FLOW_SAMPLES_MAX; 1 (the default; fv_head_set_flow(NULL) returns to it) switches it off, every size and
 * every launch is then what it was.  The sampler's rows in the workspace grow to max_samples x max_batch head rows (the higher-order solvers' two rows too),
 * so the FIRST call that names more than 1 must come before fv_bind_workspace (FV_ERR_STATE afterwards).  step_weights_host: `chunk` HOST floats, finite and
 * >= 0, the per-step weights w[k] of the coherence score (fastvla_hip.select.coherence_weights); NULL: COHERENT is refused.  chunk >= 1 divides action_dim.
 * Later calls with the same two integers may change the weights at any time (they synchronise the device).  Flow mode only (FV_ERR_STATE); FV_ERR_ARG,
 * changing nothing, outside the ranges. */
#define FV_FLOW_SAMPLES_MAX 16
#define FV_FLOW_SELECT_FIRST 0
#define FV_FLOW_SELECT_MEDOID 1
#define FV_FLOW_SELECT_COHERENT 2
int fv_head_set_flow_samples(fv_handle* h, int max_samples, int chunk, const float* step_weights_host);
/* fv_head_flow_sample (delays == NULL) or fv_head_flow_sample_prefix (delays != NULL: prefix mode, prev and shift pin as there, every candidate of a row pins
 * the same steps) for S candidates, 1 <= S <= max_samples, then the choice.  noise: (S B, action_dim) sample-major, or NULL.
 *     MEDOID    score[s] = sum over s' ascending of sum_e (x_s[e] - x_s'[e])^2
 *     COHERENT  score[s] = sum_{k < chunk - shift} w[k] sum_a (x_s[k][a] - prev[b][k + shift][a])^2; a row whose row_mask ((B) int32 or NULL) is 0 takes the
 *               MEDOID score.  A weight of 0 selects its step away; prev beyond the overlap is never read
 *     FIRST     candidate 0 (scores_out reports the MEDOID scores)
 * The smallest score wins, a non-finite score counts as +inf, ties go to the lowest index: shift == chunk, all-zero weights or no finite score choose
 * candidate 0.  A candidate with a NaN or +-inf element scores +inf in every mode and the MEDOID sums of the others leave it out: it wins only as
 * candidate 0 of a row without a finite score. chunk_out (B, action_dim) is a COPY of the chosen normalised candidate; actions (B, action_dim) applies the one fused multiply-add of the
 * folded action statistics to it, so FIRST is the single-sample call bit for bit.  Optional (NULL: not written): candidates_out (S B, action_dim) normalised,
 * sample-major; choice_out (B) int32; scores_out (B, S); spread_out (B, action_dim), the population standard deviation over the candidates per element.
 * S = 1 with every optional output NULL is the single-sample call's launches (the final stage writes actions and chunk_out itself); otherwise one launch
 * more than the single-sample call for S = 1, two more for S > 1 (the conditioning is computed on B rows and copied): no atomics, no host
 * synchronisation, no allocation, every sum in a fixed order, two calls give the same bits.  Guided sampling with candidates is not offered.
 * Refused before anything is enqueued, in fv_head_flow_sample's order: FV_ERR_STATE when flow mode is off, delays are given without prefix mode, COHERENT
 * is asked for without weights, or no workspace is bound; FV_ERR_ARG for a null flat_params / pooled / states / actions / chunk_out, prev missing where
 * delays or COHERENT need it, S outside 1 .. max_samples, an unknown select, n_steps < 1, B outside 1 .. max_batch, shift outside 0 .. chunk. */
int fv_head_flow_sample_multi(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                              uint64_t seed, uint64_t offset, int S, int select, const float* prev, int shift, const int32_t* row_mask, const int32_t* delays,
                              float* actions, float* chunk_out, float* candidates_out, int32_t* choice_out, float* scores_out, float* spread_out, fv_stream s);
/* generic backward of the head from dL/dactions (B,A) f32 (what autograd hands a custom Function when the loss is
 * computed outside, e.g. lerobot_fastvla/modeling_fastvla.py:132 + loss.backward()); overwrites flat_grads. */
int fv_head_backward(fv_handle* h, const float* flat_params, const float* grad_actions, int B, float dropout_p,
                     const void* saved, float* flat_grads, fv_stream s);
/* replaces clip_grad_norm_ + AdamW.step (training/trainer.py:60-66,178-180;
 * lerobot_fastvla/configuration_fastvla.py:51-55): fused global-norm clip + decoupled-decay Adam on the flat buffers.
 * step is 1-based.  grad_norm_out (1 f32, device, may be NULL) receives the pre-clip norm. */
int fv_adamw_clip_step(fv_handle* h, float* flat_params, const float* flat_grads, float* m, float* v, int64_t n,
                       const fv_adamw_hparams* hp, int64_t step, float* grad_norm_out, fv_stream s);

/* ---- parameter groups for the step above (torch.optim.AdamW's param_groups; the reference's trainer, training/trainer.py:60-66, has ONE group
 * because it only trains the head).  A table of groups tiles the flat buffer [0, n): each group scales the learning rate (lr_g = hp.lr * lr_scale),
 * carries its own weight decay and may be frozen.  `frozen` is what freezes a group: its elements are neither read into the clip norm nor written
 * (p, m, v keep their bits); lr_scale = 0 alone is a plain group: its gradient counts in the norm and its m / v move (p stays, the decoupled decay being lr_g * weight_decay).
 * The library cuts every group into segments of at most FV_ADAMW_SEGMENT floats, one thread block each (csrc/optim_kernels.hip). */
#define FV_ADAMW_SEGMENT 8192
typedef struct fv_adamw_group {
  int64_t begin, end;              /* [begin, end) in floats, both multiples of 4 */
  float lr_scale, weight_decay;    /* finite, >= 0 */
  int32_t frozen, reserved;        /* reserved must be 0 */
} fv_adamw_group;                  /* 32 bytes */
typedef struct fv_adamw_groups fv_adamw_groups;   /* opaque: device segment table + its partial-sum scratch */
/* A configuration call: allocates, uploads and synchronises.  FV_ERR_ARG, with a message naming the offending group, for: n <= 0 or n % 4 != 0; n_groups
 * outside 1 .. 65536; a group that is empty, unsorted, overlapping or leaves a gap; a boundary that is not a multiple of 4; the last end != n; a negative or
 * non-finite lr_scale / weight_decay; reserved != 0.  Destroy the table before the handle. */
int fv_adamw_groups_create(fv_handle* h, const fv_adamw_group* host_groups, int n_groups, int64_t n, fv_adamw_groups** out);
int fv_adamw_groups_destroy(fv_handle* h, fv_adamw_groups* groups);
/* fv_adamw_clip_step over the table: ONE global clip norm over the non-frozen elements (coefficient as fv_adamw_clip_step's), then per element the same
 * expression with lr_g and the group's weight decay -- hp->weight_decay is IGNORED by this entry.  A table whose groups all carry lr_scale 1 and one decay
 * gives fv_adamw_clip_step's p, m, v bit for bit when no clipping applies (the norm itself is summed in another fixed order).
 * grad_norm_out (1 f32, may be NULL): the pre-clip global norm; group_norms_out (n_groups f32, device, may be NULL): sqrt(group's sum of squares) * grad_scale,
 * 0 for a frozen group.  No float atomics: two runs give the same bits.  FV_ERR_ARG when n differs from the table's or a buffer is not 16-byte aligned.
 * Asynchronous on s, allocates nothing.  The table owns the partial sums, so ONE step may be in flight per table. */
int fv_adamw_clip_step_groups(fv_handle* h, float* flat_params, const float* flat_grads, float* m, float* v, int64_t n, const fv_adamw_hparams* hp,
                              const fv_adamw_groups* groups, int64_t step, float* grad_norm_out, float* group_norms_out, fv_stream s);
/* fused clip + AdamW + EMA: as fv_adamw_clip_step (groups == NULL) or fv_adamw_clip_step_groups, and ema <- ema + ema_weight (p_new - ema)
 * in the same pass.  ema: n floats, same alignment rule as flat_params on the path taken.  ema_weight in [0, 1] (1 - decay; 1 copies, 0 leaves ema alone).
 * One more read and one more write of 4 bytes per element beside the step's own traffic; p, m, v, the norm and the group norms are those of the step without
 * ema, bit for bit, and both paths give the same ema bits for the same p_new.  A frozen group's ema keeps its bits.  FV_ERR_ARG, launching nothing, for: a
 * null ema; ema overlapping flat_params, flat_grads, m or v; ema_weight outside [0, 1] or NaN; with a table, an ema that is not 16-byte aligned. */
int fv_adamw_clip_step_ema(fv_handle* h, float* flat_params, const float* flat_grads, float* m, float* v, float* ema, float ema_weight, int64_t n,
                           const fv_adamw_hparams* hp, const fv_adamw_groups* groups, int64_t step, float* grad_norm_out, float* group_norms_out, fv_stream s);

/* ---- the step guard: skip a step whose gradient is non-finite or was computed from saturated fp16 operands, and keep a dynamic loss scale, all on the
 * device (what torch.cuda.amp.GradScaler does around an optimiser: skip, back off, grow again after a run of good steps).  The guard's state is one
 * 64-byte device block:
 *   delta_log2   the dynamic factor delta = 2^delta_log2 ON TOP of the static loss scale 2^k of fv_train_set_options.  A bound guard
 *                (fv_train_set_step_guard) makes the training backward multiply dL/dactions by delta, so every gradient carries 2^k delta; the guarded step
 *                divides delta out again on the device and the caller's grad_scale = 2^-k / world / accum stays what it is.
 *   good_steps   applied steps since delta last changed
 *   the counters applied, skipped_nonfinite, skipped_saturated, saturated_applied
 *   the last decision (apply 0 / 1 and the 1 / delta that step used), the sticky saturation flag, the last value seen of the saturation counter.
 * One guarded step: the sums of squares by the kernels of the plain steps, ONE decision launch of one block, then the GUARD instance of the step kernel:
 *   bad_nonfinite = the sum of squares is not finite (a NaN / inf gradient element, or squares that overflow); a frozen group's gradient is never read
 *   bad_sat       = skip_on_saturation && flag > 0 && delta_log2 > min_delta_log2
 *   bad:  the step is SKIPPED -- p, m, v and ema keep their bits --, delta_log2 <- max(min, delta_log2 - backoff_log2), good_steps <- 0;
 *         skipped_nonfinite (which wins when both hold) or skipped_saturated counts it
 *   good: the step is applied with coef and the reported norms times 1 / delta (an exact power of two: the bits of the plain step over gradients that
 *         never carried delta; delta = 1 gives fv_adamw_clip_step[_groups | _ema]'s bits); applied counts it, saturated_applied too when the flag was set
 *         (a saturation at the floor, where halving cannot help, is applied as an unguarded run applies it); good_steps += 1, and at growth_interval
 *         delta_log2 <- min(max, delta_log2 + growth_log2), good_steps <- 0
 *   either way the flag is cleared, and grad_norm_out / group_norms_out are written (non-finite if that is what they are: the log shows why).
 * `step`, which feeds the bias correction, stays the CALLER'S count and advances on a skipped step too, as a learning-rate schedule does: a rare skip
 * shifts the bias correction by one step, and a run without skips needs no second code path.
 * No float atomics, no host read, no allocation after create; two runs give the same bits; every call below that takes a stream is capturable. */
typedef struct fv_step_guard fv_step_guard;
typedef struct fv_step_guard_config {
  int32_t init_delta_log2, min_delta_log2, max_delta_log2;
  int32_t growth_interval;             /* >= 1; GradScaler's default is 2000 */
  int32_t backoff_log2, growth_log2;   /* >= 0; 1 and 1 halve and double */
  int32_t skip_on_saturation;          /* 0: a flagged step is applied (and counted in saturated_applied) */
  int32_t reserved;                    /* must be 0 */
} fv_step_guard_config;                /* 32 bytes */
typedef struct fv_step_guard_state {
  int32_t delta_log2, good_steps;
  int32_t last_apply; float last_inv_delta;
  float flag; uint32_t last_saturations;
  int64_t applied, skipped_nonfinite, skipped_saturated, saturated_applied;
} fv_step_guard_state;                 /* 56 bytes */
/* A configuration call: allocates, uploads and synchronises.  FV_ERR_ARG for: min > max, init outside [min, max], growth_interval < 1, a negative
 * backoff_log2 / growth_log2, reserved != 0, or a range that, added to the handle's current loss_scale_log2, leaves [0, 24] (fv_train_set_options' bounds).
 * Head-only training is fp32 and has no loss scale: its guard is created with min = init = max = 0 and guards against non-finite gradients only.
 * Destroy the guard before the handle (a guard still bound to the backward is unbound by its destruction). */
int fv_step_guard_create(fv_handle* h, const fv_step_guard_config* cfg, fv_step_guard** out);
int fv_step_guard_destroy(fv_handle* h, fv_step_guard* g);
/* the state for a checkpoint / from one: status calls, both synchronise.  import: FV_ERR_ARG for a delta_log2 outside the guard's range or negative counts. */
int fv_step_guard_export(fv_handle* h, fv_step_guard* g, fv_step_guard_state* out);
int fv_step_guard_import(fv_handle* h, fv_step_guard* g, const fv_step_guard_state* in);
/* ONE one-block launch, to be enqueued after a backward: if the handle's fp16 saturation counter (the one behind fv_llm_fp16_saturations) differs from the
 * value seen last, the flag is set; the new value is remembered.  The flag is sticky across the micro-batches of a gradient-accumulation window until a
 * guarded step consumes it. */
int fv_step_guard_observe(fv_handle* h, fv_step_guard* g, fv_stream s);
/* *flag_dev <- the device address of the flag, one float holding 0 or 1: data-parallel callers SUM it across ranks before the guarded step (any value > 0
 * counts as set), so that every rank takes the same decision.  The non-finite check needs no exchange: a NaN or inf survives the gradient sum on every rank. */
int fv_step_guard_flag(fv_handle* h, fv_step_guard* g, float** flag_dev);
/* ONE one-block launch: out2_dev (2 floats, device) <- { 1 if the last guarded step was skipped, else 0; the delta the next backward runs with }: what a
 * training loop logs per step without reading anything back. */
int fv_step_guard_report(fv_handle* h, fv_step_guard* g, float* out2_dev, fv_stream s);
/* the guarded form of all four steps: ema == NULL -> no average is kept (ema_weight ignored), groups == NULL -> the single-group step, otherwise the operands
 * and their rules are fv_adamw_clip_step_ema's.  FV_ERR_ARG, launching nothing and leaving the guard's state untouched, for a null guard and for everything
 * the unguarded entry points refuse. */
int fv_adamw_clip_step_guarded(fv_handle* h, float* flat_params, const float* flat_grads, float* m, float* v, float* ema, float ema_weight, int64_t n,
                               const fv_adamw_hparams* hp, const fv_adamw_groups* groups, int64_t step, fv_step_guard* guard, float* grad_norm_out,
                               float* group_norms_out, fv_stream s);
/* bind the guard to fv_train_forward_backward / fv_train_lora_forward_backward (NULL unbinds; a configuration call like fv_train_set_tower_grad): while bound,
 * dL/dactions is multiplied by the guard's delta (one launch over its floats, read from the device) right after the loss launch, which still writes the
 * static 2^k; everything downstream is linear in that buffer.  The tower's stream picks its own power-of-two scale per step towards a target of twice the loss
 * scale; with a guard bound that target is 2^(k+1) delta, read on the device, so the stream follows the whole scale as it follows a static one, and it takes
 * only its own scale out again: the tower's gradients carry 2^k delta like every other, with the bits of a run whose static scale is 2^k delta.  Without a bound guard nothing new is launched.  FV_ERR_ARG when the guard's range
 * added to the current loss_scale_log2 leaves [0, 24]; fv_train_set_options refuses such a loss_scale_log2 while the guard is bound. */
int fv_train_set_step_guard(fv_handle* h, fv_step_guard* guard);

/* ---- temporal ensembling of action chunks (ACT's exponential weighting; LeRobot's ACTTemporalEnsembler, per environment).  Every control step the policy
 * predicts a chunk of K future steps; the action served for time t is the weighted mean of what the chunks predicted at t-K+1 .. t (those that exist since
 * the last reset) say about t:  sum_i w_i c_i[t] / sum_i w_i  with  w_i = exp(-coeff i), i = 0 the OLDEST prediction.  coeff: any finite float; 0 is
 * uniform, a negative one favours new predictions.  Kept in the online form  ens <- (ens cumsum_w[n-1] + c w[n]) / cumsum_w[n]  with a count n per slot.
 * Device state: ens (n_env, K, A) f32 and count (n_env, K) int32, a ring -- slot (t + k) mod K holds the running mean for time t + k; w and cumsum_w
 * (K floats each) are computed on the host in double, rounded once and uploaded at create.
 * THE RING POSITION t IS HOST STATE of the ensembler and travels as a kernel argument: a hipGraph captured over fv_ensemble_step bakes the position of
 * its capture in and replays it wrongly -- call fv_ensemble_step outside captured graphs. */
typedef struct fv_ensembler fv_ensembler;
/* A configuration call: allocates, uploads and synchronises.  FV_ERR_ARG for n_env, chunk or step_dim < 1, a non-finite coeff, a coeff whose weights
 * leave the fp32 range over `chunk` steps, or a null pointer.  Destroy the ensembler before the handle. */
int fv_ensemble_create(fv_handle* h, int n_env, int chunk, int step_dim, float coeff, fv_ensembler** out);
int fv_ensemble_destroy(fv_handle* h, fv_ensembler* e);
/* forget the history of environment env (-1 = all): its next step serves row 0 of the new chunk as it is.  Stream-ordered, no host synchronisation:
 * vector environments that end episodes at different times are reset one by one.  FV_ERR_ARG, nothing enqueued, for env outside -1 .. n_env-1. */
int fv_ensemble_reset(fv_handle* h, fv_ensembler* e, int env, fv_stream s);
/* chunks: DEVICE (n_env, K, A) f32, the chunks predicted now; actions: DEVICE (n_env, A) f32, the ensembled action of this time step (must not overlap
 * chunks).  ONE launch; every (env, slot) belongs to one thread: no atomics, no reduction, two runs agree bit for bit, and one environment's values
 * (NaN included) never reach another's.  A slot without history (K = 1, or the first step after a reset) returns the chunk's row bit for bit.
 * Asynchronous on s, allocates nothing; steps of one ensembler must be enqueued in order on one stream (or otherwise ordered).  FV_ERR_ARG, with nothing
 * enqueued and the state untouched, for a null pointer. */
int fv_ensemble_step(fv_handle* h, fv_ensembler* e, const float* chunks, float* actions, fv_stream s);

/* gradient accumulation (training/trainer.py:96,171: accelerate sums micro-batch gradients before the optimiser step):
 * acc += grads over n floats; both 16-byte aligned flat head buffers. */
int fv_grad_accumulate(fv_handle* h, float* acc, const float* grads, int64_t n, fv_stream s);
/* grads *= *scale_dev (a device scalar, e.g. the upstream dL/dloss autograd hands compute_loss's backward) */
int fv_grad_scale(fv_handle* h, float* grads, int64_t n, const float* scale_dev, fv_stream s);

/* ---- data-parallel exchange (replaces accelerate/DDP's gradient all-reduce, training/trainer.py:68-78,175) ---------- */
/* One RCCL communicator per rank over xGMI.  rank 0 calls fv_comm_unique_id, the host side carries the 128 bytes to every
 * rank (torch.distributed store / broadcast), every rank calls fv_comm_init.  comm is an ncclComm_t. */
int fv_comm_unique_id(fv_handle* h, fv_rccl_id* id_out);
int fv_comm_init(fv_handle* h, const fv_rccl_id* id, int rank, int world, void** comm_out);
int fv_comm_destroy(fv_handle* h, void* comm);
/* ONE all-reduce (sum, in place) of the flat head gradient on stream s; the 1/world average is fv_adamw_hparams.grad_scale */
int fv_allreduce_grads(fv_handle* h, void* comm, float* flat_grads, int64_t n, fv_stream s);

/* ---- unfrozen-backbone training ------------------------------------------------------------------------
 * The reference's knob is fastvla/configuration_fastvla.py:23 `freeze_backbone` (applied at model/fastvlm_adapter.py:170-173) and is made
 * moot there by the unconditional no_grad at model/fastvlm_adapter.py:501; the step body is training/trainer.py:60-66,171-182 over ALL
 * parameters.  This slice: Qwen2 decoder (embedding, every layer, final norm) + mm_projector + action expert trainable, FastViT-HD tower
 * frozen, image tokens SPLICED in front of the text (a text-only sequence gives the projector no gradient), last_token pooling.
 *
 * All trainable parameters live in ONE caller-owned flat fp32 buffer (the master copy; same for gradients and Adam's m / v):
 *   [ action expert (fv_head_layout) | projector | embedding | layer 0 .. L-1 | final norm ]
 * with every matrix in the layout the library packs it in: q | k | v rows concatenated (packing 1), gate / up rows interleaved in blocks of
 * 8 ([8 gate | 8 up], packing 2).  fv_train_layout lists every tensor (name, element offset, rows x cols, gradient bucket, packing). */
typedef struct fv_train_tensor {
  char name[104];   /* canonical checkpoint key; packed tensors: "...self_attn.qkv_proj.{weight,bias}", "...mlp.gate_up_proj.weight" */
  int64_t offset, numel;
  int32_t rows, cols;
  int32_t bucket;   /* 0 = action expert, 1 = projector, 2 = embedding, 3 + l = decoder layer l, 3 + L = final norm */
  int32_t packing;  /* 0 = plain [rows][cols], 1 = q|k|v concatenated along rows, 2 = gate/up rows interleaved by 8 */
} fv_train_tensor;
/* out may be NULL (sizes only).  n_buckets = 3 + llm_layers + 1. */
int fv_train_layout(fv_handle* h, fv_train_tensor* out, int max_tensors, int* n_tensors, int64_t* total_numel, int* n_buckets);
/* one-time: allocates the library-owned transposed bf16 weight copies the dgrad GEMMs read.  Needs llm_precision = 1, head_dim 64 / 128. */
int fv_train_begin(fv_handle* h);
/* backbone part of the flat master buffer <- the library's current weights (the head part is the caller's) */
int fv_train_export_params(fv_handle* h, float* flat_params, fv_stream s);
/* the library's MFMA operand copies <- the master, after an optimiser step: bf16 weights (RNE), their transposes, fp32 norms / biases.
 * The frozen-path entry points (fv_llm_forward_pooled, ...) see the updated weights from then on. */
int fv_train_commit(fv_handle* h, const float* flat_params, fv_stream s);
/* Arithmetic of the backward's contractions (defaults 2, 1, 12: every dgrad and wgrad ONE fp16 pass -- worst per-tensor gradient 8.4e-4 from fp32 autograd
 * through the whole 24-layer 0.5B decoder, 6.7e-4 at the 7B width; in this mode the gate/up accumulators are kept as fp16 for the backward):
 *   grad_split 2: ONE fp16 pass -- the loss-scaled gradient rounded once to 11 significant bits against an fp16 copy of the transposed weight (exact:
 *                 bf16 widens into fp16);
 *              1: the gradient operand of every dgrad GEMM is split bf16 (hi + lo, 16 significant bits) against the exact-bf16 transposed weights
 *                 (two passes; the most exact form: 3.3e-4 through all 24 layers).
 *   wgrad_f16  1: every weight gradient in ONE fp16 pass -- the gradient and the activation each rounded once to 11 significant bits (operands as
 *                 transposed fp16 copies, made where the data is produced);
 *              0: the split-bf16 gradient against the activation's bf16 hi half (two passes; the activation's 8 bits bound the result at ~1.8e-3).
 *   (Round 5 removed grad_split 0 -- plain-bf16 gradient operands, 3.7e-3: outside the 2e-3 bar -- and wgrad_f16 2 -- the decoder's wgrads on the TN GEMM
 *   instance: same gradients, 1 ms per step slower.  The TN instance lives on in the tower's weight gradients, whose contraction runs over 10^5 .. 10^6 pixel rows.)
 *   loss_scale_log2: dL/dactions is multiplied by 2^k, so EVERY gradient fv_train_forward_backward writes carries that factor (it keeps the wgrad's
 *              fp16 gradient operand inside binary16's range; saturating casts, clamps counted by fv_llm_fp16_saturations); pass
 *              grad_scale = 2^-k / world to fv_adamw_clip_step (fv_train_loss_scale returns 2^k).  The loss itself is not scaled. */
int fv_train_set_options(fv_handle* h, int grad_split, int wgrad_f16, int loss_scale_log2);
int fv_train_loss_scale(fv_handle* h, float* scale_out);
/* on != 0: the TRAINING forward's four projections per layer in ONE fp16 pass (normed rows / attention output / SwiGLU output rounded once to 11 significant bits
 * against exact fp16 copies of the bf16 weights; down's copy carries 2^4) instead of the split-bf16 form's two -- half the forward's MFMA work; everything the
 * backward differentiates is kept as before.  The inference entry points do not change.  Needs the default fp16 backward.
 * OPT-IN, outside the 1e-3 bar: through all 24 layers of the 0.5B decoder actions sit 1.0e-3 and gradients up to 2.1e-3 from fp32 autograd (default forward:
 * 1.2e-5 / 8.4e-4; tests/test_gpu_train_unfrozen.py). */
int fv_train_set_forward_f16(fv_handle* h, int on);
int fv_train_workspace_bytes(fv_handle* h, int B, int T, size_t* out_bytes);
/* called from inside fv_train_forward_backward, on the calling thread, right after the LAST kernel that writes bucket `bucket`'s gradient
 * has been enqueued on the stream: flat_grads[offset, offset + numel) is final once the stream reaches this point (record an event here and
 * start that bucket's all-reduce on a side stream: it runs under the rest of the backward pass).  Order: 0, 3 + L, 3 + L - 1, ..., 3, 2, 1. */
typedef void (*fv_bucket_cb)(void* user, int bucket, int64_t offset, int64_t numel);
/* ONE training step's forward + MSE + backward over every trainable tensor (replaces model.compute_loss + accelerator.backward,
 * training/trainer.py:173-175, for an unfrozen backbone):
 *   tower_out (B, Ni, tower_out_dim) bf16 = the frozen tower's embeddings (fv_vision_forward's tower_out); ids (B, T) int32 right-padded,
 *   T % 8 == 0; lens (B); states (B, state_dim), targets (B, action_dim) f32; training / dropout as fv_head_forward.
 *   -> actions (B, action_dim) (normalised space), loss (1 f32, device), flat_grads (overwritten: every tensor of fv_train_layout, TIMES the
 *      loss scale of fv_train_set_options -- 2^12 by default).
 * ws: caller-owned scratch of fv_train_workspace_bytes(B, T) bytes (every activation the backward needs is kept there: no recompute).
 * Asynchronous on s; allocates nothing; gradients are bit-reproducible (no float atomics). */
int fv_train_forward_backward(fv_handle* h, const float* flat_params, const void* tower_out, const int32_t* ids, const int32_t* lens,
                              const float* states, const float* targets, int B, int T, int training, float dropout_p, uint64_t seed,
                              uint64_t offset, void* ws, size_t ws_bytes, float* actions, float* loss, float* flat_grads, fv_bucket_cb cb,
                              void* user, fv_stream s);

/* ---- the TOWER half of the slice (FastViT-HD trainable too; csrc/tower_train.inc).  After fv_train_begin:
 * fv_train_tower_begin appends the tower's tensors (inference form: folded RepMixer / ConvFFN convolutions, fc1 / fc2, layer scales, attention, PatchEmbed,
 * stem, conv_exp + SE) to the flat master -- fv_train_layout then lists them after "model.norm.weight" (packing 3 = depthwise weights tap-major [k*k][C],
 * 4 = the stem's dense 3x3 as [27][C0] with row (ky*3+kx)*3+ci; new gradient buckets 3 + L + 1 ...: stem, then per stage [blocks (+RepCPE)] [PatchEmbed],
 * last conv_exp + SE) -- and fv_train_export_params / fv_train_commit cover them (commit refreshes every packed operand image the kernels read).
 * One step: fv_train_tower_forward (pixels -> tower_out, every unit's tensors kept in tws) -> fv_train_forward_backward with fv_train_set_tower_grad's buffer
 * bound (it then also leaves dL/d(tower_out) there, fp16 [B][tokens][tower_out_dim], loss-scaled) -> fv_train_tower_backward (tower gradients into the same
 * flat_grads, cb per tower bucket in backward order).  pix must stay alive between the two tower calls. */
int fv_train_tower_begin(fv_handle* h);
int fv_train_tower_workspace_bytes(fv_handle* h, int B, size_t* out_bytes);
int fv_train_tower_forward(fv_handle* h, const void* pix, int B, void* tws, size_t tws_bytes, void* tower_out, fv_stream s);
/* Binds (NULL: unbinds) the buffer fv_train_forward_backward leaves dL/d(tower_out) in.  That gradient carries a power-of-two scale of its own, chosen on the device every
 * step and taken out again by fv_train_tower_backward.  A CHANGE of binding resets the scale to 1 (a configuration call: it synchronises the device); binding the buffer
 * that is already bound is a no-op, so a training loop may call this every step.  A caller that fills a gradient buffer ITSELF and hands it to fv_train_tower_backward
 * (no fv_train_forward_backward in between) must have changed the binding since the last fv_train_forward_backward -- e.g. bind NULL first, as the unit tests do. */
int fv_train_set_tower_grad(fv_handle* h, void* d_tower_out_f16);
int fv_train_tower_backward(fv_handle* h, const void* pix, const void* d_tower_out_f16, int B, void* tws, size_t tws_bytes, float* flat_grads, fv_bucket_cb cb,
                            void* user, fv_stream s);
/* ONE tower unit, teacher-forced (parity tests): forward of unit `unit` (fv_vision_unit_info's index; the unit count itself = conv_exp + SE) on x_in (bf16 NHWC;
 * the stem: fv_preprocess pixels), then its backward from g_out (fp32 NHWC, dL/d(output)) x gscale.  y_out (bf16, optional) = the unit's output, g_in (fp32,
 * optional; ignored for the stem) = dL/d(input), the unit's weight gradients x gscale at their fv_train_layout offsets in flat_grads. */
/* unit `unit`'s output (bf16 NHWC) as the last fv_train_tower_forward left it in tws */
int fv_train_tower_read_unit(fv_handle* h, int unit, int B, const void* tws, size_t tws_bytes, void* out, fv_stream s);
int fv_train_tower_unit(fv_handle* h, int unit, const void* x_in, const float* g_out, float gscale, int B, void* tws, size_t tws_bytes, void* y_out, float* g_in,
                        float* flat_grads, fv_stream s);

/* ---- LoRA mode of the slice above (csrc/lora_path.inc, csrc/lora_kernels.hip).  The reference has no adapter mode: this extends its one knob
 * (fastvla/configuration_fastvla.py:23 `freeze_backbone`) and its step body (training/trainer.py:60-66,171-182: clip_grad_norm_ + AdamW over the parameters
 * with requires_grad) to the usual way a VLM of this size is fine-tuned: the decoder's matrices stay FROZEN in the fp32 master and every target matrix runs as
 *     W' = W0 + s * B @ A        s = alpha / rank,  A (rank x in),  B (out x rank)                   (PEFT's merged LoRA, no dropout)
 * while the action expert and the mm_projector train in full.  The TRAINABLE parameters live in a flat fp32 buffer of their own (gradients and Adam's m / v
 * mirror THAT buffer; the full-size m / v are never needed):
 *     [ action expert | projector | layer 0 adapters .. layer L-1 adapters ]
 * head and projector at the offsets fv_train_layout gives them (the two buffers share their front), adapters per LOGICAL matrix in PEFT's names
 * ("model.layers.{l}.self_attn.q_proj.lora_A.weight" (rank x in), "...lora_B.weight" (out x rank), "...mlp.gate_proj...", ...), plain row-major.
 * One step:  fv_train_forward_backward (unchanged: the full dW' into the full gradient buffer)  ->  fv_train_lora_project  ->  all-reduce + ONE
 * fv_adamw_clip_step over the trainable buffer (its clip norm is over exactly the trainable tensors)  ->  fv_train_lora_commit.
 * All four calls below that take a stream are asynchronous on it and allocate nothing. */
enum fv_lora_target { FV_LORA_Q = 1, FV_LORA_K = 2, FV_LORA_V = 4, FV_LORA_O = 8, FV_LORA_GATE = 16, FV_LORA_UP = 32, FV_LORA_DOWN = 64, FV_LORA_ALL = 127 };
/* after fv_train_begin.  rank 1 .. 64, alpha > 0, target_mask a non-empty set of fv_lora_target bits (FV_ERR_ARG otherwise); FV_ERR_UNSUPPORTED after
 * fv_train_tower_begin (tower adapters do not exist; fv_train_tower_begin refuses after this call in turn).  Allocates the descriptor tables and the
 * projection's scratch once; a second call with the same arguments is a no-op, with others FV_ERR_STATE. */
int fv_train_lora_begin(fv_handle* h, int rank, float alpha, int target_mask);
/* fv_train_lora_begin with variants (fv_train_lora_begin == flags 0; anything but these two bits FV_ERR_ARG; beginning again with other flags FV_ERR_STATE):
 *   FV_LORA_RSLORA  rank-stabilised scaling: s = alpha / sqrt(rank).  Nothing else changes; both backward modes work.
 *   FV_LORA_DORA    weight-decomposed LoRA (PEFT's use_dora):  W' = diag(m / n) @ V,  V = W0 + s * B @ A,  n_i = ||V_i,:||_2,  m a TRAINED magnitude per output
 *                   row.  The layout lists "....lora_magnitude_vector.weight" (1 x out) behind each target's lora_B; head and projector keep their offsets.
 *                   The norm is a constant in the backward (PEFT, the DoRA paper section 4.3): with G = dW', c = m / n
 *                       dm_i = (sum_j G_ij V_ij) / n_i        dA = s * B^T @ diag(c) @ G        dB = s * diag(c) @ G @ A^T
 *                   fv_train_lora_commit refreshes n into a buffer the handle owns and remembers the master it read; fv_train_lora_project uses both, so it
 *                   MUST FOLLOW A COMMIT OF THE SAME PARAMETERS (FV_ERR_STATE when no commit has run; a stale one goes unnoticed).  fv_train_lora_merge
 *                   writes diag(c) @ V.  fv_train_lora_forward_backward answers FV_ERR_UNSUPPORTED (dm from activations needs the pre-bias GEMM outputs). */
enum fv_lora_flags { FV_LORA_DORA = 1, FV_LORA_RSLORA = 2 };
int fv_train_lora_begin_ex(fv_handle* h, int rank, float alpha, int target_mask, int flags);
/* DoRA only (FV_ERR_STATE otherwise): every magnitude in lora_params <- the row norm of W0 + s * B @ A for the A, B it holds, by the kernel and summation order
 * the commit uses -- so m / n is exactly 1.0f and the commit that follows builds the operand images a commit without the magnitude would (with lora_B = 0:
 * fv_train_commit's own; m = ||W0|| per row, PEFT's initialisation).  Also after fv_train_lora_merge, with lora_B zeroed, on the merged master. */
int fv_train_lora_init_magnitude(fv_handle* h, const float* flat_params_master, float* lora_params, fv_stream s);
/* the trainable buffer's tensors (packing 0 throughout; bucket 0 head, 1 projector, 3 + l the adapters of layer l).  out may be NULL (sizes only). */
int fv_train_lora_layout(fv_handle* h, fv_train_tensor* out, int max_tensors, int* n_tensors, int64_t* total_numel);
/* lora_grads (trainable layout) <- the full gradient buffer fv_train_forward_backward filled: head and projector gradients copied, and for every adapted matrix
 *     dA = s * B^T @ dW'        dB = s * dW' @ A^T
 * from ONE read of dW' (ranks above 32: two), in fp32 on the f32-input matrix core, summed in a fixed order (bit-reproducible).  The loss scale dW' carries
 * passes straight through (fv_adamw_clip_step's grad_scale removes it as in the full mode). */
int fv_train_lora_project(fv_handle* h, const float* flat_grads_full, const float* lora_params, float* lora_grads, fv_stream s);
/* fv_train_commit in LoRA mode: the operand images of every adapted matrix from W0 + s * B @ A (evaluated in fp32, then rounded as fv_train_commit rounds W0),
 * every other tensor as fv_train_commit.  Head and projector are taken from lora_params: the master's head | projector FRONT is overwritten with theirs (that is
 * where fv_train_forward_backward reads the head); nothing else of the master is written -- W0 stays as it is.
 * With FV_LORA_DORA the commit also refreshes the row norms and KEEPS the pointer flat_params_master: the next fv_train_lora_project reads W0 through it, so that
 * buffer must stay allocated, in place and unchanged behind its front until that projection has run (a freed, moved or re-filled master goes unnoticed). */
int fv_train_lora_commit(fv_handle* h, float* flat_params_master, const float* lora_params, fv_stream s);
/* W0 += s * B @ A into the master, for every adapted matrix (and its front <- lora_params' front): bit for bit the fp32 values fv_train_lora_commit rounds, so
 * fv_train_commit on the merged master builds the same operand images.  For exporting a plain checkpoint; the adapters are not reset. */
int fv_train_lora_merge(fv_handle* h, float* flat_params_master, const float* lora_params, fv_stream s);
/* The DIRECT LoRA step: fv_train_forward_backward's forward and input-gradient chain, with the weight gradients of the decoder replaced by
 *     P = dY @ B,  Q = X @ A^T,  dA = s * P^T @ X,  dB = s * dY^T @ Q        (csrc/lora_direct_kernels.hip: fp32 throughout, fixed summation order)
 * per adapted matrix, straight from the gradient's fp16 rows and the kept activations: dW' is never formed and NO full-size gradient buffer exists.  lora_grads
 * (trainable layout, overwritten, TIMES the loss scale) receives the head and projector gradients in its front and dA / dB of every adapter; the embedding, norm and
 * qkv-bias gradients and dW' of every decoder matrix are not computed, nor are the transposed operand copies that only a weight-gradient GEMM reads.  flat_params is the
 * master (its head | projector front as fv_train_lora_commit left it), lora_params the trainable buffer (B and A are read from it).  fv_train_lora_project is not
 * called in this mode; the rest of the step (all-reduce, fv_adamw_clip_step, fv_train_lora_commit) is unchanged, and so is the workspace (fv_train_workspace_bytes).
 * Needs fv_train_lora_begin (FV_ERR_STATE otherwise) and refuses with FV_ERR_UNSUPPORTED, before anything is enqueued: backward options other than the default
 * fv_train_set_options(2, 1, k), fv_train_set_forward_f16.  (A trained tower never gets here: fv_train_lora_begin and fv_train_tower_begin exclude each other.)
 * The first call allocates the kernels' scratch (sized for max_batch). */
int fv_train_lora_forward_backward(fv_handle* h, const float* flat_params, const float* lora_params, const void* tower_out, const int32_t* ids, const int32_t* lens,
                                   const float* states, const float* targets, int B, int T, int training, float dropout_p, uint64_t seed, uint64_t offset, void* ws,
                                   size_t ws_bytes, float* actions, float* loss, float* lora_grads, fv_stream s);

/* ---- optional per-kernel-family HIP-event timing (bench.py roofline numbers) ------------------------------------- */
enum fv_family { FV_FAM_GEMM = 0, FV_FAM_DWCONV, FV_FAM_STEM, FV_FAM_ATTN, FV_FAM_NORM, FV_FAM_ELT, FV_FAM_HEAD, FV_FAM_COUNT };
typedef struct fv_profile_entry { double ms, flops, bytes; int64_t launches; } fv_profile_entry;
typedef struct fv_gemm_profile { int32_t m, n, k, epi; double ms; int64_t launches; } fv_gemm_profile;
/* enable != 0: every launch the engine issues is bracketed by hipEvents on the caller's stream (algorithmic flops and
 * bytes recorded beside it).  fv_profile_read synchronises those events, fills fam_out[FV_FAM_COUNT] and up to max_gemm
 * distinct GEMM shapes, and clears the record list. */
int fv_profile(fv_handle* h, int enable);
int fv_profile_read(fv_handle* h, fv_profile_entry* fam_out, fv_gemm_profile* gemm_out, int max_gemm, int* n_gemm);

/* The op-level entry points of the parity tests (fv_op_*: one kernel each) are NOT part of this library: they are declared in
 * include/fastvla_hip_testops.h and built into vla-from-fastvlm_amd/testops/libfastvla_hip_testops.so by `make` (csrc/ops_api.hip). */

#ifdef __cplusplus
}
#endif
#endif /* FASTVLA_HIP_H */
