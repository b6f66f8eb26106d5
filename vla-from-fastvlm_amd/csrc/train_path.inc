// train_path.inc -- host side of the UNFROZEN-backbone training slice (SURVEY.md section 8f-4), included by engine.hip.
//
// Scope of the slice: Qwen2 decoder (all layers, embedding, final norm) + mm_projector + action expert trainable; FastViT-HD tower
// frozen; image tokens spliced in front of the text (in the reference-literal text-only sequence the projector gets no gradient at
// all).  The reference never reaches this path (model/fastvlm_adapter.py:501 is an unconditional no_grad; the knob it nominally has is
// fastvla/configuration_fastvla.py:23 `freeze_backbone`, handled at model/fastvlm_adapter.py:170-173): the arithmetic is torch
// autograd's over the forward this library already computes, and the step body is training/trainer.py:171-182 over ALL parameters.
//
// Parameters.  ONE flat fp32 buffer (caller-owned, like the head's): [action expert | projector | embedding | layer 0 .. L-1 | final
// norm], every matrix in the layout the library packs it in (q|k|v rows concatenated, gate/up rows interleaved by 8) so that the
// master copy, the gradient, Adam's m / v and the all-reduce all see the same contiguous array and the MFMA operand copies are made
// by a cast (fv_train_commit: master -> bf16 weights + their transposes for dgrad).  fv_train_layout names every tensor, its offset
// and its gradient BUCKET; fv_train_forward_backward calls `cb` the moment a bucket's gradient is complete (head, final norm, layer
// L-1 .. 0, embedding, projector), which is where the host side hangs one all-reduce per bucket on a side stream under the rest of
// the backward pass.
//
// Arithmetic.  Forward = the library's parity-mode decoder (split-bf16 operands, fp32 norms / residual; attention on the bf16 matrix core
// with split operands, attention_split.hip) with every tensor the backward needs kept in the caller's workspace; the SwiGLU runs in the
// gate/up GEMM's epilogue, which also keeps its raw accumulators.  Backward: fp32 residual-gradient stream carrying 2^loss_scale_log2 from
// the loss on; each dgrad / wgrad is ONE launch of the forward's GEMM kernels.  Default (fv_train_set_options 2, 1, 12): both operands
// rounded once to fp16 (the gradient as rows for the dgrad and as columns for the wgrad, made from one read; the transposed weights as
// exact fp16 copies of the bf16 weights; the activations' columns), one pass each -- half the MFMA work of the split form this path
// started with and more exact than it (8.4e-4 against 1.8e-3 worst per-tensor gradient); the other options keep the split-bf16 /
// plain-bf16 forms for comparison.  Everything else fp32 (train_kernels.hip); no atomics on any gradient.

namespace {

struct TrainTensor {
  std::string name;
  int64_t off = 0, numel = 0;
  int rows = 1, cols = 0, bucket = 0, packing = 0;
  void* lib = nullptr;      // the library's own copy (bf16 matrix or fp32 vector); null for the head (caller-owned only)
  bool is_mat = false;
  bf16_t** tcopy = nullptr; // where the transposed bf16 copy lives (dgrad operand), matrices of the decoder / projector.2 only
  bf16_t** tcopy16 = nullptr; // ... and its fp16 twin
  bf16_t** row16 = nullptr;   // fp16 row copy x scale16 (the one-pass fp16 training forward), decoder projections only
  float scale16 = 1.0f;
};

enum { TB_HEAD = 0, TB_PROJ = 1, TB_EMBED = 2, TB_LAYER0 = 3 };

// tower_train.inc (the tower half of the slice): its tensors are appended behind the decoder's once fv_train_tower_begin has run
void append_tower_tensors(fv_handle* h, std::vector<TrainTensor>& out, int64_t& off);
int tower_export(fv_handle* h, float* flat, hipStream_t s);
int tower_bucket_count(const fv_handle* h);
// lora_path.inc (the LoRA mode): its commit tables name the same operand copies as fv_train_commit's and are rebuilt with it
int build_lora_tables(fv_handle* h);
int lora_direct_call(fv_handle* h, int l, int which, const bf16_t* dY16, const bf16_t* X, int xkind, int ldx, int lo_off, int R, const float* lora_params,
                     float* lora_grads, hipStream_t s);

std::vector<TrainTensor> train_tensors(fv_handle* h, int64_t* total) {
  const fv_model_desc& d = h->d;
  std::vector<TrainTensor> out;
  int64_t off = 0;
  auto add = [&](const std::string& n, int rows, int cols, int bucket, void* lib, bool mat, int packing = 0, bf16_t** tc = nullptr, bf16_t** tc16 = nullptr) {
    TrainTensor t;
    t.name = n; t.off = off; t.rows = rows; t.cols = cols; t.numel = (int64_t)rows * cols; t.bucket = bucket; t.lib = lib; t.is_mat = mat;
    t.packing = packing; t.tcopy = tc; t.tcopy16 = tc16;
    off += (t.numel + 3) / 4 * 4;
    out.push_back(t);
  };
  static const char* head_names[12] = {"state_projection.0.weight", "state_projection.0.bias", "state_projection.1.weight", "state_projection.1.bias",
                                       "fusion.0.weight", "fusion.0.bias", "fusion.1.weight", "fusion.1.bias", "fusion.4.weight", "fusion.4.bias",
                                       "action_head.weight", "action_head.bias"};
  const fv::HeadOffsets ho = fv::head_offsets(h->hd);
  const fv::HeadDims& hd = h->hd;
  const int hrows[12] = {1, 1, hd.hid, 1, hd.fus, 1, 1, 1, hd.fus, 1, hd.da, 1};
  const int hcols[12] = {hd.ds, hd.ds, hd.ds, hd.hid, hd.feat + hd.hid, hd.fus, hd.fus, hd.fus, hd.fus, hd.fus, hd.fus, hd.da};
  for (int i = 0; i < 12; ++i) {
    TrainTensor t;
    t.name = head_names[i]; t.off = ho.o[i]; t.rows = hrows[i]; t.cols = hcols[i]; t.numel = (int64_t)t.rows * t.cols; t.bucket = TB_HEAD;
    out.push_back(t);
  }
  off = (ho.o[12] + 3) / 4 * 4;
  const int H = d.llm_hidden, CO = d.tower_out_dim, I = d.llm_inter, D = d.llm_head_dim;
  const int qd = d.llm_heads * D, kd = d.llm_kv_heads * D, qkvw = qd + 2 * kd;
  Tower& tw = h->tw;
  add("model.mm_projector.0.weight", H, CO, TB_PROJ, tw.pj0_w, true, 0, h->train.tower ? &h->train.pj0T : nullptr, h->train.tower ? &h->train.pj0T16 : nullptr);
  add("model.mm_projector.0.bias", 1, H, TB_PROJ, tw.pj0_b, false);
  add("model.mm_projector.2.weight", H, H, TB_PROJ, tw.pj2_w, true, 0, &h->train.pj2T, &h->train.pj2T16);
  add("model.mm_projector.2.bias", 1, H, TB_PROJ, tw.pj2_b, false);
  add("model.embed_tokens.weight", d.llm_vocab, H, TB_EMBED, h->dec.embed, true);
  for (size_t l = 0; l < h->dec.layers.size(); ++l) {
    DecLayer& L = h->dec.layers[l];
    const std::string pre = "model.layers." + std::to_string(l) + ".";
    const int b = TB_LAYER0 + (int)l;
    TrainLayerT* T = h->train.layers.size() > l ? &h->train.layers[l] : nullptr;
    add(pre + "input_layernorm.weight", 1, H, b, L.ln1, false);
    add(pre + "self_attn.qkv_proj.weight", qkvw, H, b, L.qkv_w, true, 1, T ? &T->qkvT : nullptr, T ? &T->qkvT16 : nullptr);   // rows: q | k | v
    if (T) out.back().row16 = &T->qkv16;
    add(pre + "self_attn.qkv_proj.bias", 1, qkvw, b, L.qkv_b, false, 1);
    add(pre + "self_attn.o_proj.weight", H, qd, b, L.o_w, true, 0, T ? &T->oT : nullptr, T ? &T->oT16 : nullptr);
    if (T) out.back().row16 = &T->o16;
    add(pre + "post_attention_layernorm.weight", 1, H, b, L.ln2, false);
    add(pre + "mlp.gate_up_proj.weight", 2 * I, H, b, L.gu_w, true, 2, T ? &T->guT : nullptr, T ? &T->guT16 : nullptr);      // rows: [8 gate | 8 up] blocks
    if (T) out.back().row16 = &T->gu16;
    add(pre + "mlp.down_proj.weight", H, I, b, L.down_w, true, 0, T ? &T->downT : nullptr, T ? &T->downT16 : nullptr);
    if (T) { out.back().row16 = &T->down16; out.back().scale16 = 16.0f; }
  }
  add("model.norm.weight", 1, H, TB_LAYER0 + (int)h->dec.layers.size(), h->dec.norm, false);
  if (h->train.tower) append_tower_tensors(h, out, off);
  if (total) *total = off;
  return out;
}

struct TrainPlan {
  int B, T, Ni, Tt, rows, Rp, RI, RIp;
  size_t x_in, x_mid, xn1, qkvf, att, lse, xn2, gu, act;    // per-layer stashes: offset of layer 0, strides below
  size_t s_x, s_xn, s_qkvf, s_att, s_lse, s_gu, s_act, apart;
  size_t pre0, hsplit, tok;                                   // projector stash
  size_t act_s, dx, dtmp, dsplit, AT, XT, dqkv, attn_scr, delta, scr, pooled, dpooled, xg, dxg, head_saved, head_scr, splitk;
  size_t splitk_bytes, total;
  size_t wmax;   // the widest gradient operand (columns): the dsplit scratch holds rows x 3 wmax 16-bit values
};

TrainPlan plan_train(const fv_handle* h, int B, int T) {
  const fv_model_desc& d = h->d;
  TrainPlan p{};
  const int side = d.image_size >> (d.tower_stages + 1);
  p.B = B; p.T = T; p.Ni = side * side; p.Tt = p.Ni + T; p.rows = B * p.Tt; p.Rp = (p.rows + 63) / 64 * 64; p.RI = B * p.Ni; p.RIp = (p.RI + 63) / 64 * 64;
  const size_t L = d.llm_layers, H = d.llm_hidden, I = d.llm_inter, D = d.llm_head_dim, CO = d.tower_out_dim;
  const size_t qd = d.llm_heads * D, qkvw = qd + 2 * d.llm_kv_heads * D, rows = p.rows, Rp = p.Rp;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes); return r; };
  p.s_x = align_up(rows * H * 4); p.s_xn = align_up(rows * 2 * H * 2); p.s_qkvf = align_up(rows * qkvw * 4); p.s_att = align_up(rows * 2 * qd * 2);
  p.s_lse = align_up((size_t)B * d.llm_heads * p.Tt * 4); p.s_gu = align_up(rows * 2 * I * 4);
  p.x_in = take(p.s_x * (L + 1)); p.x_mid = take(p.s_x * L); p.xn1 = take(p.s_xn * L); p.qkvf = take(p.s_qkvf * L); p.att = take(p.s_att * L);
  p.lse = take(p.s_lse * L); p.xn2 = take(p.s_xn * L); p.gu = take(p.s_gu * L);
  p.s_act = align_up(rows * 2 * I * 2); p.act = take(p.s_act * L);      // silu(gate) * up as [hi | lo] bf16: the down projection's operand, forward and wgrad
  p.apart = take((size_t)(d.llm_heads / d.llm_kv_heads) * rows * 2 * d.llm_kv_heads * D * 4);   // per-q-head shares of dK / dV (attn_bwd_dkv_kernel<PART>)
  p.pre0 = take((size_t)p.RI * H * 4); p.hsplit = take((size_t)p.RI * 2 * H * 2); p.tok = take((size_t)p.RI * H * 4);
  const size_t wmax = std::max(std::max(2 * I, qkvw), H);                 // widest gradient operand (columns)
  const size_t xmax = std::max(std::max(std::max(I, H), qd), CO);         // widest activation operand (columns)
  const size_t rmax = std::max((size_t)Rp, (size_t)p.RIp);
  p.act_s = 0;
  p.dx = take(rows * H * 4);
  p.dtmp = take(std::max(rows * std::max(std::max(I, H), qd), (size_t)p.RI * CO) * 4);   // (also dL/d(tower_out) in fp32 on its way to the tower's backward)
  p.wmax = wmax;
  p.dsplit = take(rows * 3 * wmax * 2);   // the split-bf16 rows of the widest gradient operand, and room for its fp16 rows behind them
  p.AT = take(wmax * 2 * rmax * 2);
  p.XT = take(xmax * rmax * 2);
  p.dqkv = take(rows * qkvw * 4);
  p.attn_scr = take(fv::attention_split_scratch_bytes(B, p.Tt, d.llm_kv_heads, d.llm_head_dim));   // K / V records of the split-bf16 attention kernels
  p.delta = take(p.s_lse);
  p.scr = take((fv::rmsnorm_bwd_scratch_floats(rows, (int)H) + (size_t)fv::COLSUM_CHUNKS * std::max(qkvw, H)) * 4);
  p.pooled = take((size_t)B * H * 4); p.dpooled = take((size_t)B * H * 4); p.xg = take((size_t)B * H * 4); p.dxg = take((size_t)B * H * 4);
  p.head_saved = take(fv::head_saved_bytes(h->hd, B));
  p.head_scr = take(fv::head_bwd_scratch_bytes(h->hd, B));
  // split-K partial sums: up to 4 K ranges of the widest fp32 output cut that way (rows x pad(max(H, qkvw)) forward / dgrad, a weight
  // gradient [<= 2I][<= pad(I)] backward); launch_gemm takes as many ranges as fit
  p.splitk_bytes = (size_t)4 * std::max(rows * ((std::max(H, qkvw) + 255) / 256 * 256), std::max(H, qkvw) * ((I + 255) / 256 * 256)) * 4;
  p.splitk = take(p.splitk_bytes);
  p.total = o;
  return p;
}

#define TR_GEMM(...)                       \
  do {                                     \
    fv::GemmArgs _g{__VA_ARGS__};          \
    FV_TRY(gemm_p(h, _g, s));              \
  } while (0)

// dW[N][K] (fp32, into the flat gradient) = dY^T . X over `R` rows: dY fp32 [R][ldy] (N columns), X bf16 [R][ldx] (K columns, the hi
// half of a split operand) or bf16-exact; both transposed into the scratch operands first
// (dYs != null: the gradient already as split bf16 [R][2N] = [hi | lo] -- its two halves are transposed on their own)
// (at_ready: the fp16 transposed gradient already sits in the AT scratch -- launch_swiglu_bwd_f16 wrote it)
// at_ptr: where that transposed gradient sits (default: the start of the AT scratch); xt_ready: the transposed fp16 activation is in the XT scratch already
int wgrad(fv_handle* h, const TrainPlan& tp, char* ws, const float* dY, int ldy, int N, const bf16_t* X, int ldx, int K, int R, float* dW, hipStream_t s,
          const bf16_t* dYs = nullptr, bool at_ready = false, bf16_t* at_ptr = nullptr, bool xt_ready = false, int xkind = -1) {   // xkind 3: X holds fp16 rows
  const int Rp = (R + 63) / 64 * 64;
  const int sp = h->train.grad_split;   // 0: the gradient's bf16 hi half alone (one pass)
  bf16_t* AT = at_ptr ? at_ptr : reinterpret_cast<bf16_t*>(ws + tp.AT);
  bf16_t* XT = reinterpret_cast<bf16_t*>(ws + tp.XT);
  if (h->train.wgrad_f16) {
    // ONE fp16 pass: the (loss-scaled) gradient and the activation both rounded ONCE to 11 significant bits -- 2e-4 per tensor where the
    // split-bf16 gradient against the bf16 (8-bit) activation gave 1.8e-3, at half the MFMA work.  X: the split operand's halves summed first.
    if (at_ready) {}
    else if (dYs) FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_transpose_to_f16(dYs, 2, 2 * N, N, AT, Rp, R, Rp, N, h->f16_flags, s));
    else FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_transpose_to_f16(dY, 0, ldy, 0, AT, Rp, R, Rp, N, h->f16_flags, s));
    if (!xt_ready) FV_P(FV_FAM_ELT, 0.0, (double)R * K * 6, fv::launch_transpose_to_f16(X, xkind >= 0 ? xkind : (ldx >= 2 * K ? 2 : 1), ldx, K, XT, Rp, R, Rp, K, h->f16_flags, s));
    fv::GemmArgs g16{AT, Rp, XT, N, K, Rp, nullptr, nullptr, nullptr, 0, dW, K, FV_EPI_F32, 0};
    g16.f16 = 1;
    g16.splitk_ws = tp.splitk_bytes ? reinterpret_cast<float*>(ws + tp.splitk) : nullptr;
    g16.splitk_bytes = tp.splitk_bytes;
    FV_TRY(gemm_p(h, g16, s));
    return FV_OK;
  }
  if (dYs) {
    FV_P(FV_FAM_ELT, 0.0, (double)R * N * 4, fv::launch_transpose_to_bf16(dYs, 1, 2 * N, AT, 2 * Rp, 0, R, Rp, N, s));
    if (sp) FV_P(FV_FAM_ELT, 0.0, (double)R * N * 4, fv::launch_transpose_to_bf16(dYs + N, 1, 2 * N, AT + Rp, 2 * Rp, 0, R, Rp, N, s));
  } else
  FV_P(FV_FAM_ELT, 0.0, (double)R * N * 8, fv::launch_transpose_to_bf16(dY, 0, ldy, AT, 2 * Rp, sp ? Rp : 0, R, Rp, N, s));
  FV_P(FV_FAM_ELT, 0.0, (double)R * K * 4, fv::launch_transpose_to_bf16(X, 1, ldx, XT, Rp, 0, R, Rp, K, s));
  fv::GemmArgs g{AT, 2 * Rp, XT, N, K, Rp, nullptr, nullptr, nullptr, 0, dW, K, FV_EPI_F32, sp};
  // few output tiles over a contraction as long as the batch (o_proj: 4 x 4 tiles, K = 2 x 10240): cut along K, one unit per CU
  g.splitk_ws = tp.splitk_bytes ? reinterpret_cast<float*>(ws + tp.splitk) : nullptr;
  g.splitk_bytes = tp.splitk_bytes;
  FV_TRY(gemm_p(h, g, s));
  return FV_OK;
}

// dX[R][K] (fp32) = dY[R][N] . W[N][K] through the transposed weight copy WT [K][N]
// (dY16: the gradient's fp16 rows [R][N], already made)
int dgrad(fv_handle* h, const TrainPlan& tp, char* ws, const float* dY, int ldy, int N, const bf16_t* WT, int K, int R, float* dX, hipStream_t s,
          const bf16_t* dYs = nullptr, const bf16_t* WT16 = nullptr, const bf16_t* dY16 = nullptr) {
  const bf16_t* ds = dYs;
  const int sp = h->train.grad_split;
  if (sp == 2) {   // ONE fp16 pass: the (loss-scaled) gradient rounded once to 11 bits against the fp16 copy of the transposed weight (exact: bf16 widens into fp16)
    bf16_t* d16 = reinterpret_cast<bf16_t*>(ws + tp.dsplit);
    bf16_t* dst = dYs ? d16 + (size_t)R * 2 * N : d16;   // (a pre-split operand lives in the same scratch: the fp16 rows go behind it)
    if (dY16) dst = const_cast<bf16_t*>(dY16);
    else if (dYs) FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_rows_to_f16(dYs, 2, 2 * N, N, dst, N, R, N, h->f16_flags, s));
    else FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_rows_to_f16(dY, 0, ldy, 0, dst, N, R, N, h->f16_flags, s));
    fv::GemmArgs g16{dst, N, WT16, R, K, N, nullptr, nullptr, nullptr, 0, dX, K, FV_EPI_F32, 0};
    g16.f16 = 1;
    g16.splitk_ws = tp.splitk_bytes ? reinterpret_cast<float*>(ws + tp.splitk) : nullptr;
    g16.splitk_bytes = tp.splitk_bytes;
    FV_TRY(gemm_p(h, g16, s));
    return FV_OK;
  }
  if (!ds) {
    bf16_t* dsw = reinterpret_cast<bf16_t*>(ws + tp.dsplit);
    FV_P(FV_FAM_ELT, 0.0, (double)R * N * 8, fv::launch_split_rows(dY, ldy, dsw, 2 * N, sp ? N : 0, R, N, s));
    ds = dsw;
  }
  fv::GemmArgs g{ds, 2 * N, WT, R, K, N, nullptr, nullptr, nullptr, 0, dX, K, FV_EPI_F32, sp};
  g.splitk_ws = tp.splitk_bytes ? reinterpret_cast<float*>(ws + tp.splitk) : nullptr;
  g.splitk_bytes = tp.splitk_bytes;
  FV_TRY(gemm_p(h, g, s));
  return FV_OK;
}

// one-pass fp16 arithmetic on both sides (the defaults): an fp32 gradient's dgrad operand (fp16 rows, in the dsplit scratch) and wgrad operand (fp16
// columns, at `at`) from ONE read of it
bool fp16_backward(const fv_handle* h) { return h->train.grad_split == 2 && h->train.wgrad_f16; }
int grad_operands(fv_handle* h, const TrainPlan& tp, char* ws, const float* dY, int ldy, int N, int R, bf16_t* at, hipStream_t s) {
  const int Rp = (R + 63) / 64 * 64;
  FV_P(FV_FAM_ELT, 0.0, (double)R * N * 8,
       fv::launch_transpose_to_f16(dY, 0, ldy, 0, at, Rp, R, Rp, N, h->f16_flags, s, reinterpret_cast<bf16_t*>(ws + tp.dsplit), N));
  return FV_OK;
}

// fv_train_commit's descriptor table: one launch refreshes every operand copy of the decoder / projector from the master
int build_commit_table(fv_handle* h) {
  std::vector<fv::CommitDesc> cd;
  int tiles = 0;
  for (const TrainTensor& t : train_tensors(h, nullptr)) {
    if (!t.lib) continue;
    fv::CommitDesc c{};
    c.src_off = t.off; c.dst = t.lib; c.is_mat = t.is_mat ? 1 : 0; c.tile0 = tiles;
    if (t.is_mat) {
      if (t.cols % 8 || t.rows % 8) return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_begin: %s is %d x %d (dimensions must be multiples of 8)", t.name.c_str(), t.rows, t.cols);
      c.rows = t.rows; c.cols = t.cols;
      c.dstT16 = t.tcopy16 ? *t.tcopy16 : nullptr; c.dstTb = t.tcopy ? *t.tcopy : nullptr;
      c.dst16 = (h->train.fwd_f16 && t.row16) ? *t.row16 : nullptr; c.scale16 = t.scale16;
      tiles += ((t.rows + 63) / 64) * ((t.cols + 63) / 64);
    } else {
      c.rows = 1; c.cols = (int)t.numel;
      tiles += (int)((t.numel + 4095) / 4096);
    }
    cd.push_back(c);
  }
  void* dp = nullptr;
  FV_TRY(dev_alloc(h, cd.size() * sizeof(fv::CommitDesc), &dp));
  FV_HIP_CHECK(hipMemcpy(dp, cd.data(), cd.size() * sizeof(fv::CommitDesc), hipMemcpyHostToDevice));
  h->train.commit_desc = static_cast<fv::CommitDesc*>(dp); h->train.commit_n = (int)cd.size(); h->train.commit_tiles = tiles;
  if (h->train.lora.on) FV_TRY(build_lora_tables(h));
  return FV_OK;
}

int train_check(fv_handle* h) {
  FV_TRY(check_ready(h, false));
  if (!h->train.ready) return fv_fail(FV_ERR_STATE, "unfrozen training not initialised: call fv_train_begin first");
  return FV_OK;
}

}  // namespace

extern "C" {

int fv_train_layout(fv_handle* h, fv_train_tensor* out, int max_tensors, int* n_tensors, int64_t* total_numel, int* n_buckets) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  int64_t total = 0;
  const std::vector<TrainTensor> tt = train_tensors(h, &total);
  if (n_tensors) *n_tensors = (int)tt.size();
  if (total_numel) *total_numel = total;
  if (n_buckets) *n_buckets = TB_LAYER0 + h->d.llm_layers + 1 + (h->train.tower ? tower_bucket_count(h) : 0);
  if (out) {
    if (max_tensors < (int)tt.size()) return fv_fail(FV_ERR_ARG, "fv_train_layout: room for %d tensors, %zu needed", max_tensors, tt.size());
    for (size_t i = 0; i < tt.size(); ++i) {
      memset(&out[i], 0, sizeof(out[i]));
      snprintf(out[i].name, sizeof(out[i].name), "%s", tt[i].name.c_str());
      out[i].offset = tt[i].off; out[i].numel = tt[i].numel; out[i].rows = tt[i].rows; out[i].cols = tt[i].cols;
      out[i].bucket = tt[i].bucket; out[i].packing = tt[i].packing;
    }
  }
  return FV_OK;
}

int fv_train_begin(fv_handle* h) {
  HandleScope _hs(h);
  FV_TRY(check_ready(h, false));
  const fv_model_desc& d = h->d;
  if (d.llm_precision != 1) return fv_fail(FV_ERR_UNSUPPORTED, "unfrozen training needs llm_precision = 1 (bf16 weight copies; fp16 copies cannot be refreshed from the master)");
  if (d.llm_head_dim != 64 && d.llm_head_dim != 128) return fv_fail(FV_ERR_UNSUPPORTED, "unfrozen training: llm head_dim must be 64 or 128");
  if (d.llm_hidden > 4096 || d.llm_hidden % 64 || (2 * d.llm_inter) % 64 || ((d.llm_heads + 2 * d.llm_kv_heads) * d.llm_head_dim) % 64)
    return fv_fail(FV_ERR_UNSUPPORTED, "unfrozen training: hidden (<= 4096), 2 * inter and the packed qkv width must be multiples of 64");
  if (h->train.ready) return FV_OK;
  FV_HIP_CHECK(hipSetDevice(h->device));
  const size_t H = d.llm_hidden, I = d.llm_inter, D = d.llm_head_dim, qd = d.llm_heads * D, qkvw = qd + 2 * d.llm_kv_heads * D;
  h->train.layers.resize(h->dec.layers.size());
  void* p = nullptr;
  for (TrainLayerT& T : h->train.layers) {
    FV_TRY(dev_alloc(h, qkvw * H * 2, &p)); T.qkvT = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, H * qd * 2, &p)); T.oT = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, 2 * I * H * 2, &p)); T.guT = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, H * I * 2, &p)); T.downT = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, qkvw * H * 2, &p)); T.qkvT16 = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, H * qd * 2, &p)); T.oT16 = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, 2 * I * H * 2, &p)); T.guT16 = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, H * I * 2, &p)); T.downT16 = static_cast<bf16_t*>(p);
  }
  FV_TRY(dev_alloc(h, H * H * 2, &p)); h->train.pj2T = static_cast<bf16_t*>(p);
  FV_TRY(dev_alloc(h, H * H * 2, &p)); h->train.pj2T16 = static_cast<bf16_t*>(p);
  // transposed copies of the weights as loaded: bf16 (split / plain dgrad) and fp16 (one-pass dgrad; bf16 widens into fp16 exactly)
  for (const TrainTensor& t : train_tensors(h, nullptr))
    if (t.tcopy) {
      FV_TRY(fv::launch_transpose_to_bf16(t.lib, 1, t.cols, *t.tcopy, t.rows, 0, t.rows, t.rows, t.cols, nullptr));
      FV_TRY(fv::launch_transpose_to_f16(t.lib, 1, t.cols, 0, *t.tcopy16, t.rows, t.rows, t.rows, t.cols, h->f16_flags, nullptr));
    }
  FV_TRY(build_commit_table(h));
  FV_HIP_CHECK(hipDeviceSynchronize());
  h->train.ready = true;
  return FV_OK;
}

// backbone part of the flat master buffer <- the library's current weights (bf16 matrices widen exactly; fp32 vectors copy)
int fv_train_export_params(fv_handle* h, float* flat, fv_stream st) {
  HandleScope _hs(h);
  FV_TRY(train_check(h));
  if (!flat) return fv_fail(FV_ERR_ARG, "fv_train_export_params: null buffer");
  hipStream_t s = static_cast<hipStream_t>(st);
  for (const TrainTensor& t : train_tensors(h, nullptr)) {
    if (!t.lib) continue;
    if (t.is_mat) FV_TRY(fv::launch_bf16_to_f32(static_cast<const bf16_t*>(t.lib), flat + t.off, (size_t)t.numel, s));
    else FV_HIP_CHECK(hipMemcpyAsync(flat + t.off, t.lib, (size_t)t.numel * 4, hipMemcpyDeviceToDevice, s));
  }
  if (h->train.tower) FV_TRY(tower_export(h, flat, s));
  return FV_OK;
}

// the library's operand copies <- the master (after an optimiser step): bf16 weights (round to nearest even), their transposes, fp32 vectors
int fv_train_commit(fv_handle* h, const float* flat, fv_stream st) {
  HandleScope _hs(h);
  FV_TRY(train_check(h));
  if (!flat) return fv_fail(FV_ERR_ARG, "fv_train_commit: null buffer");
  hipStream_t s = static_cast<hipStream_t>(st);
  // (the transposed copies of the ACTIVE dgrad form only: fp16 for grad_split = 2, bf16 otherwise -- fv_train_set_options rebuilds the other on a switch)
  FV_TRY(fv::launch_commit(h->train.commit_desc, h->train.commit_n, h->train.commit_tiles, flat, h->train.grad_split == 2 ? 1 : 0, h->f16_flags, s));
  if (h->train.tower) FV_TRY(fv::launch_tower_commit(h->train.tower_ops, h->train.tower_nops, h->train.tower_blocks, flat, h->f16_flags, s));
  return FV_OK;
}

int fv_train_set_options(fv_handle* h, int grad_split, int wgrad_f16, int loss_scale_log2) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  // (round 5: grad_split = 0 -- plain-bf16 gradient operands, 3.7e-3, outside the bar -- and wgrad_f16 = 2 -- the decoder's wgrads on the TN GEMM instance, same
  // gradients, 1 ms slower -- are gone from the product; the TN instance itself serves the tower's weight gradients, tower_train.inc)
  if (grad_split < 1 || grad_split > 2 || wgrad_f16 < 0 || wgrad_f16 > 1 || loss_scale_log2 < 0 || loss_scale_log2 > 24)
    return fv_fail(FV_ERR_ARG, "fv_train_set_options: grad_split in {1, 2}, wgrad_f16 in {0, 1}, loss_scale_log2 in [0, 24]");
  if (h->train.ready && ((grad_split == 2) != (h->train.grad_split == 2))) {
    // the transposed weight copies of the OTHER form may be stale (fv_train_commit refreshes the active form only): rebuild them from the library's weights
    FV_HIP_CHECK(hipSetDevice(h->device));
    FV_HIP_CHECK(hipDeviceSynchronize());
    for (const TrainTensor& t : train_tensors(h, nullptr)) {
      if (!t.tcopy) continue;
      if (grad_split == 2) FV_TRY(fv::launch_transpose_to_f16(t.lib, 1, t.cols, 0, *t.tcopy16, t.rows, t.rows, t.rows, t.cols, h->f16_flags, nullptr));
      else FV_TRY(fv::launch_transpose_to_bf16(t.lib, 1, t.cols, *t.tcopy, t.rows, 0, t.rows, t.rows, t.cols, nullptr));
    }
    FV_HIP_CHECK(hipDeviceSynchronize());
  }
  h->train.grad_split = grad_split;
  h->train.wgrad_f16 = wgrad_f16 != 0;
  h->train.loss_scale_log2 = loss_scale_log2;
  return FV_OK;
}
int fv_train_loss_scale(fv_handle* h, float* scale_out) {
  HandleScope _hs(h);
  if (!h || !scale_out) return fv_fail(FV_ERR_ARG, "null argument");
  *scale_out = std::ldexp(1.0f, h->train.loss_scale_log2);
  return FV_OK;
}

// on != 0: the TRAINING forward's projections (qkv, o, gate/up, down) in ONE fp16 pass against fp16 copies of the weights instead of the split-bf16 form's two
// passes (the inference entry points are untouched).  Allocates the fp16 row copies on first use; fv_train_commit keeps them fresh while the mode is on.
int fv_train_set_forward_f16(fv_handle* h, int on) {
  HandleScope _hs(h);
  FV_TRY(train_check(h));
  if (!on) { if (h->train.fwd_f16) { h->train.fwd_f16 = false; FV_TRY(build_commit_table(h)); } return FV_OK; }
  FV_HIP_CHECK(hipSetDevice(h->device));
  FV_HIP_CHECK(hipDeviceSynchronize());
  for (const TrainTensor& t : train_tensors(h, nullptr)) {
    if (!t.row16) continue;
    if (!*t.row16) { void* p = nullptr; FV_TRY(dev_alloc(h, (size_t)t.numel * 2, &p)); *t.row16 = static_cast<bf16_t*>(p); }
    // from the library's current bf16 weights: copy, then widen in place (exact; down x 2^4)
    FV_HIP_CHECK(hipMemcpy(*t.row16, t.lib, (size_t)t.numel * 2, hipMemcpyDeviceToDevice));
    FV_TRY(fv::launch_bf16_to_f16(*t.row16, (size_t)t.numel, t.scale16, nullptr, h->f16_flags + 1));
  }
  FV_HIP_CHECK(hipDeviceSynchronize());
  unsigned bits = 0;
  FV_HIP_CHECK(hipMemcpy(&bits, h->f16_flags + 1, 4, hipMemcpyDeviceToHost));
  float mx;
  memcpy(&mx, &bits, 4);
  if (!(mx <= 65504.0f)) return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_set_forward_f16: a projection weight leaves the fp16 range (max |w| x scale = %g; down carries x16)", (double)mx);
  h->train.fwd_f16 = true;
  FV_TRY(build_commit_table(h));
  return FV_OK;
}

int fv_train_workspace_bytes(fv_handle* h, int B, int T, size_t* out_bytes) {
  HandleScope _hs(h);
  if (!h || !out_bytes) return fv_fail(FV_ERR_ARG, "null argument");
  if (B <= 0 || T <= 0 || T % 8) return fv_fail(FV_ERR_ARG, "fv_train_workspace_bytes: B > 0 and T a positive multiple of 8");
  if ((long)B * T > 16384) return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_workspace_bytes: %ld text positions per step (the embedding gradient keeps the batch's ids in 64 KB of LDS: B * T <= 16384)", (long)B * T);
  *out_bytes = plan_train(h, B, T).total;
  return FV_OK;
}

// ONE body for fv_train_forward_backward and fv_train_lora_forward_backward (lora_path.inc).  lora_grads != null selects the DIRECT LoRA backward: the same forward
// and dgrad chain; the head and projector gradients go to lora_grads (same offsets); every decoder weight gradient is replaced by lora_direct_call (dA, dB straight
// from the gradient's fp16 rows and the kept activation) or dropped (embedding, norms, qkv bias, matrices without an adapter), the fp16 COLUMN copies of gradient and
// activation are not made, and flat_grads does not exist.
static int train_forward_backward_impl(fv_handle* h, const float* flat_params, const void* tower_out_v, const int32_t* ids, const int32_t* lens,
                                       const float* states, const float* targets, int B, int T, int training, float dropout_p, uint64_t seed,
                                       uint64_t offset, void* ws_v, size_t ws_bytes, float* actions, float* loss, float* flat_grads, fv_bucket_cb cb,
                                       void* user, fv_stream st, const float* lora_params, float* lora_grads) {
  HandleScope _hs(h);
  TrainScope _ts(h);
  FV_TRY(train_check(h));
  const bool direct = lora_grads != nullptr;
  const char* who = direct ? "fv_train_lora_forward_backward" : "fv_train_forward_backward";
  float* gbuf = direct ? lora_grads : flat_grads;    // where the head's and the projector's gradients go (the two layouts share their front)
  if (!flat_params || !tower_out_v || !ids || !lens || !states || !targets || !ws_v || !actions || !loss || !gbuf)
    return fv_fail(FV_ERR_ARG, "%s: null pointer", who);
  const fv_model_desc& d = h->d;
  if (B <= 0 || B > d.max_batch || T <= 0 || T % 8 || T > d.max_text_tokens) return fv_fail(FV_ERR_ARG, "%s: bad B / T (T must be a multiple of 8)", who);
  // refused HERE, before anything is enqueued or any bucket's all-reduce is launched (launch_embed_bwd runs at the very end of the backward).  The direct LoRA
  // backward computes no embedding gradient, but fv_train_workspace_bytes sizes the workspace for both entry points and admits no larger step: same limit, its own words
  if (direct && (long)B * T > 16384)
    return fv_fail(FV_ERR_UNSUPPORTED, "%s: %ld text positions per step (fv_train_workspace_bytes admits B * T <= 16384)", who, (long)B * T);
  if ((long)B * T > 16384) return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_forward_backward: %ld text positions per step (the embedding gradient keeps the batch's ids in 64 KB of LDS: B * T <= 16384)", (long)B * T);
  const TrainPlan tp = plan_train(h, B, T);
  if (tp.total > ws_bytes) return fv_fail(FV_ERR_STATE, "training workspace too small (%zu > %zu)", tp.total, ws_bytes);
  if (((uintptr_t)ws_v | (uintptr_t)gbuf | (uintptr_t)flat_params) & 15) return fv_fail(FV_ERR_ARG, "%s: buffers must be 16-byte aligned", who);
  if (tp.Tt > h->rope_rows) return fv_fail(FV_ERR_ARG, "sequence of %d tokens exceeds the RoPE table (%d)", tp.Tt, h->rope_rows);
  hipStream_t s = static_cast<hipStream_t>(st);
  char* ws = static_cast<char*>(ws_v);
  const bf16_t* tower_out = static_cast<const bf16_t*>(tower_out_v);
  const int H = d.llm_hidden, I = d.llm_inter, I2 = 2 * I, D = d.llm_head_dim, CO = d.tower_out_dim;
  const int qd = d.llm_heads * D, kd = d.llm_kv_heads * D, qkvw = qd + 2 * kd;
  const int rows = tp.rows, RI = tp.RI, Ni = tp.Ni, Tt = tp.Tt, L = (int)h->dec.layers.size();
  const float att_scale = 1.0f / std::sqrt((float)D);
  int64_t total = 0;
  const std::vector<TrainTensor> tt = train_tensors(h, &total);
  auto G = [&](const std::string& name) -> float* {
    for (const TrainTensor& t : tt) if (t.name == name) return (direct && t.bucket > TB_PROJ) ? nullptr : gbuf + t.off;   // direct: no gradient behind the projector
    return nullptr;
  };
  auto bucket_done = [&](int bucket) {
    if (!cb) return;
    int64_t lo = INT64_MAX, hi = 0;
    for (const TrainTensor& t : tt) if (t.bucket == bucket) { lo = std::min(lo, t.off); hi = std::max(hi, t.off + (t.numel + 3) / 4 * 4); }
    if (bucket == TB_HEAD) { lo = 0; hi = (fv::head_offsets(h->hd).o[12] + 3) / 4 * 4; }   // the head's own layout (and its padding)
    cb(user, bucket, lo, hi - lo);
  };
  auto X_in = [&](int l) { return reinterpret_cast<float*>(ws + tp.x_in + tp.s_x * l); };
  auto X_mid = [&](int l) { return reinterpret_cast<float*>(ws + tp.x_mid + tp.s_x * l); };
  auto XN1 = [&](int l) { return reinterpret_cast<bf16_t*>(ws + tp.xn1 + tp.s_xn * l); };
  auto XN2 = [&](int l) { return reinterpret_cast<bf16_t*>(ws + tp.xn2 + tp.s_xn * l); };
  auto QKV = [&](int l) { return reinterpret_cast<float*>(ws + tp.qkvf + tp.s_qkvf * l); };
  auto ATT = [&](int l) { return reinterpret_cast<bf16_t*>(ws + tp.att + tp.s_att * l); };
  auto LSE = [&](int l) { return reinterpret_cast<float*>(ws + tp.lse + tp.s_lse * l); };
  auto GU = [&](int l) { return reinterpret_cast<float*>(ws + tp.gu + tp.s_gu * l); };
  auto ACT = [&](int l) { return reinterpret_cast<bf16_t*>(ws + tp.act + tp.s_act * l); };
  float* apart = reinterpret_cast<float*>(ws + tp.apart);
  bf16_t* dsplit = reinterpret_cast<bf16_t*>(ws + tp.dsplit);
  float* pre0 = reinterpret_cast<float*>(ws + tp.pre0);
  bf16_t* hsplit = reinterpret_cast<bf16_t*>(ws + tp.hsplit);
  float* tok = reinterpret_cast<float*>(ws + tp.tok);
  float* dx = reinterpret_cast<float*>(ws + tp.dx);
  float* dtmp = reinterpret_cast<float*>(ws + tp.dtmp);
  float* dqkv = reinterpret_cast<float*>(ws + tp.dqkv);
  float* delta = reinterpret_cast<float*>(ws + tp.delta);
  float* scr = reinterpret_cast<float*>(ws + tp.scr);
  float* pooled = reinterpret_cast<float*>(ws + tp.pooled);
  float* dpooled = reinterpret_cast<float*>(ws + tp.dpooled);
  float* xg = reinterpret_cast<float*>(ws + tp.xg);
  float* dxg = reinterpret_cast<float*>(ws + tp.dxg);
  float* head_saved = reinterpret_cast<float*>(ws + tp.head_saved);
  float* head_scr = reinterpret_cast<float*>(ws + tp.head_scr);
  float* splitk = tp.splitk_bytes ? reinterpret_cast<float*>(ws + tp.splitk) : nullptr;
  float* colscr = scr + fv::rmsnorm_bwd_scratch_floats(rows, H);
  Tower& tw = h->tw;

  // ------------------------------------------------------------------------------------------------ forward (everything kept)
  TR_GEMM(tower_out, CO, tw.pj0_w, RI, H, CO, tw.pj0_b, nullptr, nullptr, 0, pre0, H, FV_EPI_F32, 0);
  FV_P(FV_FAM_ELT, 20.0 * RI * H, 8.0 * RI * H, fv::launch_gelu_fwd(pre0, hsplit, 2 * H, H, RI, H, s));
  TR_GEMM(hsplit, 2 * H, tw.pj2_w, RI, H, H, tw.pj2_b, nullptr, nullptr, 0, tok, H, FV_EPI_F32, 1);
  FV_P(FV_FAM_ELT, 0.0, 6.0 * rows * H, fv::launch_embed_gather(ids, h->dec.embed, tok, X_in(0), B, T, Ni, H, d.llm_vocab, s));
  const bool f16fwd = h->train.fwd_f16;
  if (f16fwd && !fp16_backward(h)) return fv_fail(FV_ERR_UNSUPPORTED, "the fp16 training forward goes with the default one-pass fp16 backward (fv_train_set_options 2, 1, k)");
  for (int l = 0; l < L && f16fwd; ++l) {
    // ONE fp16 pass per projection (fv_train_set_forward_f16): the normed rows leave the RMSNorm as fp16, the attention output is rounded once from its split form,
    // the SwiGLU output leaves the gate/up epilogue as fp16 (x 2^-4, the down copy carries the 2^4); weights = exact fp16 copies of the bf16 weights.  The
    // accumulators the backward differentiates (qkv fp32, gate/up stash, lse) and the fp32 residual stream are kept exactly as in the split-bf16 form.
    const DecLayer& Lw = h->dec.layers[l];
    const TrainLayerT& Tw = h->train.layers[l];
    FV_P(FV_FAM_NORM, 4.0 * rows * H, 6.0 * rows * H, fv::launch_rmsnorm(X_in(l), Lw.ln1, XN1(l), nullptr, H, rows, H, d.rms_eps, s, 1, h->f16_flags));
    {
      fv::GemmArgs q1{XN1(l), H, Tw.qkv16, rows, qkvw, H, Lw.qkv_b, nullptr, nullptr, 0, QKV(l), qkvw, FV_EPI_F32, 0};
      q1.f16 = 1; q1.splitk_ws = splitk; q1.splitk_bytes = tp.splitk_bytes;
      FV_TRY(gemm_p(h, q1, s));
    }
    FV_P(FV_FAM_ATTN, 2.0 * B * (double)Tt * Tt * qd, 4.0 * rows * (qkvw + qd),
         fv::launch_attention_f32(QKV(l), qkvw, ATT(l), ATT(l) + qd, 2 * qd, B, Tt, d.llm_heads, d.llm_kv_heads, D, lens, Ni, att_scale, s, h->rope, nullptr, 0, 0, LSE(l), 0, ws + tp.attn_scr));
    FV_P(FV_FAM_ELT, 0.0, (double)rows * qd * 6, fv::launch_rows_to_f16(ATT(l), 2, 2 * qd, qd, dsplit, qd, rows, qd, h->f16_flags, s));
    {
      fv::GemmArgs o1{dsplit, qd, Tw.o16, rows, H, qd, nullptr, nullptr, X_in(l), H, X_mid(l), H, FV_EPI_RES_F32, 0};
      o1.f16 = 1; o1.splitk_ws = splitk; o1.splitk_bytes = tp.splitk_bytes;
      FV_TRY(gemm_p(h, o1, s));
    }
    FV_P(FV_FAM_NORM, 4.0 * rows * H, 6.0 * rows * H, fv::launch_rmsnorm(X_mid(l), Lw.ln2, XN2(l), nullptr, H, rows, H, d.rms_eps, s, 1, h->f16_flags));
    {
      fv::GemmArgs g1{XN2(l), H, Tw.gu16, rows, I2, H, nullptr, nullptr, nullptr, 0, ACT(l), I, FV_EPI_SWIGLU_F16, 0};
      g1.f16 = 1; g1.stash = GU(l); g1.stash_f16 = 1; g1.sat = h->f16_flags;
      FV_TRY(gemm_p(h, g1, s));
    }
    {
      fv::GemmArgs d1{ACT(l), I, Tw.down16, rows, H, I, nullptr, nullptr, X_mid(l), H, X_in(l + 1), H, FV_EPI_RES_F32, 0};
      d1.f16 = 1; d1.splitk_ws = splitk; d1.splitk_bytes = tp.splitk_bytes;
      FV_TRY(gemm_p(h, d1, s));
    }
  }
  for (int l = 0; l < L && !f16fwd; ++l) {
    const DecLayer& Lw = h->dec.layers[l];
    FV_P(FV_FAM_NORM, 4.0 * rows * H, 8.0 * rows * H, fv::launch_rmsnorm(X_in(l), Lw.ln1, XN1(l), XN1(l) + H, 2 * H, rows, H, d.rms_eps, s));
    {
      fv::GemmArgs q1{XN1(l), 2 * H, Lw.qkv_w, rows, qkvw, H, Lw.qkv_b, nullptr, nullptr, 0, QKV(l), qkvw, FV_EPI_F32, 1};
      q1.splitk_ws = splitk; q1.splitk_bytes = tp.splitk_bytes;
      FV_TRY(gemm_p(h, q1, s));
    }
    FV_P(FV_FAM_ATTN, 2.0 * B * (double)Tt * Tt * qd, 4.0 * rows * (qkvw + qd),
         fv::launch_attention_f32(QKV(l), qkvw, ATT(l), ATT(l) + qd, 2 * qd, B, Tt, d.llm_heads, d.llm_kv_heads, D, lens, Ni, att_scale, s, h->rope, nullptr, 0, 0, LSE(l), 0, ws + tp.attn_scr));
    {
      fv::GemmArgs o1{ATT(l), 2 * qd, Lw.o_w, rows, H, qd, nullptr, nullptr, X_in(l), H, X_mid(l), H, FV_EPI_RES_F32, 1};
      o1.splitk_ws = splitk; o1.splitk_bytes = tp.splitk_bytes;
      FV_TRY(gemm_p(h, o1, s));
    }
    FV_P(FV_FAM_NORM, 4.0 * rows * H, 8.0 * rows * H, fv::launch_rmsnorm(X_mid(l), Lw.ln2, XN2(l), XN2(l) + H, 2 * H, rows, H, d.rms_eps, s));
    {   // gate/up with the SwiGLU in its epilogue (act leaves as the down projection's split operand) AND the raw accumulators kept for the backward
      fv::GemmArgs g1{XN2(l), 2 * H, Lw.gu_w, rows, I2, H, nullptr, nullptr, nullptr, 0, ACT(l), I2, FV_EPI_SWIGLU_SPLIT, 1};
      g1.stash = GU(l);
      // the one-pass fp16 backward rounds d gate/up and act to fp16 operands anyway: it keeps the accumulators as fp16 too (the epilogue of this
      // launch is write-bound: 600 -> 400 MB; the SwiGLU backward reads 200 MB less)
      g1.stash_f16 = fp16_backward(h) ? 1 : 0; g1.sat = h->f16_flags;
      FV_TRY(gemm_p(h, g1, s));
    }
    {
      fv::GemmArgs d1{ACT(l), I2, Lw.down_w, rows, H, I, nullptr, nullptr, X_mid(l), H, X_in(l + 1), H, FV_EPI_RES_F32, 1};
      d1.splitk_ws = splitk; d1.splitk_bytes = tp.splitk_bytes;
      FV_TRY(gemm_p(h, d1, s));
    }
  }
  FV_P(FV_FAM_ELT, 4.0 * B * H, 8.0 * B * H, fv::launch_pool_norm(X_in(L), lens, h->dec.norm, pooled, B, Tt, Ni, H, d.rms_eps, 0, s));
  const fv::HeadIoNorm* io = h->has_io ? &h->io : nullptr;
  // training != 0: the loss lives in normalised action space (fv_head_forward's convention)
  FV_P(FV_FAM_HEAD, 0.0, 0.0, fv::launch_head_forward(h->hd, flat_params, pooled, states, B, training ? (dropout_p > 0.f ? 1 : 2) : 2, dropout_p, seed, offset, actions,
                                                     head_saved, s, io));

  // ------------------------------------------------------------------------------------------------ backward
  FV_P(FV_FAM_HEAD, 0.0, 0.0, fv::launch_head_backward(h->hd, flat_params, nullptr, actions, targets, B, dropout_p, head_saved, loss, gbuf, head_scr, s, dpooled,
                                                      std::ldexp(1.0f, h->train.loss_scale_log2)));
  bucket_done(TB_HEAD);
  // final norm on the pooled rows; the residual-gradient stream starts as zero everywhere else
  FV_TRY(fv::launch_pool_rows(X_in(L), xg, lens, B, Tt, Ni, H, 0, s));
  FV_TRY(fv::launch_rmsnorm_bwd(xg, h->dec.norm, dpooled, nullptr, dxg, G("model.norm.weight"), scr, B, H, d.rms_eps, s));
  FV_HIP_CHECK(hipMemsetAsync(dx, 0, (size_t)rows * H * 4, s));
  FV_TRY(fv::launch_pool_rows(dx, dxg, lens, B, Tt, Ni, H, 1, s));
  bucket_done(TB_LAYER0 + L);
  for (int l = L - 1; l >= 0; --l) {
    const DecLayer& Lw = h->dec.layers[l];
    const TrainLayerT& Tw = h->train.layers[l];
    const std::string pre = "model.layers." + std::to_string(l) + ".";
    // down projection: x_out = x_mid + act . Wd^T
    if (direct) {
      // gradient ROWS only (no column copies: nothing here runs a weight-gradient GEMM).  dx's fp16 rows go into the last third of the dsplit scratch, so that they
      // outlive the SwiGLU backward, which writes d gate/up's rows at its start and silu(gate) * up as fp16 rows (the down adapters' activation) into the XT scratch
      bf16_t* dx16 = dsplit + (size_t)rows * 2 * tp.wmax;
      bf16_t* act16 = reinterpret_cast<bf16_t*>(ws + tp.XT);
      FV_P(FV_FAM_ELT, 0.0, (double)rows * H * 6, fv::launch_rows_to_f16(dx, 0, H, 0, dx16, H, rows, H, h->f16_flags, s));
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, H, Tw.downT, I, rows, dtmp, s, nullptr, Tw.downT16, dx16));  // d act [rows][I]
      FV_P(FV_FAM_ELT, 18.0 * rows * I, 16.0 * rows * I, fv::launch_swiglu_bwd_rows(GU(l), 1, dtmp, rows, rows, I, dsplit, act16, h->f16_flags, s));
      FV_TRY(lora_direct_call(h, l, 3, dx16, act16, 3, I, 0, rows, lora_params, lora_grads, s));
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, I2, Tw.guT, H, rows, dtmp, s, nullptr, Tw.guT16, dsplit)); // d xn2 [rows][H]
      FV_TRY(lora_direct_call(h, l, 2, dsplit, XN2(l), 2, 2 * H, H, rows, lora_params, lora_grads, s));
    } else if (fp16_backward(h)) {
      // dx -> fp16 rows + columns in one pass; d act; then the SwiGLU backward writes d gate/up straight into the two fp16 operands its consumers
      // read (rows for the dgrad, columns for the wgrad) AND act^T for the down projection's wgrad, which therefore runs after it
      bf16_t* at0 = reinterpret_cast<bf16_t*>(ws + tp.AT);
      bf16_t* at1 = at0 + (size_t)I2 * tp.Rp;   // behind the widest gradient's columns
      FV_TRY(grad_operands(h, tp, ws, dx, H, H, rows, at1, s));
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, H, Tw.downT, I, rows, dtmp, s, nullptr, Tw.downT16, dsplit));  // d act [rows][I]
      FV_P(FV_FAM_ELT, 18.0 * rows * I, 22.0 * rows * I,
           fv::launch_swiglu_bwd_f16(GU(l), 1, dtmp, rows, tp.Rp, I, dsplit, at0, h->f16_flags, s, reinterpret_cast<bf16_t*>(ws + tp.XT)));
      FV_TRY(wgrad(h, tp, ws, nullptr, 0, H, nullptr, 0, I, rows, G(pre + "mlp.down_proj.weight"), s, nullptr, true, at1, true));
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, I2, Tw.guT, H, rows, dtmp, s, nullptr, Tw.guT16, dsplit)); // d xn2 [rows][H]
      FV_TRY(wgrad(h, tp, ws, nullptr, 0, I2, XN2(l), f16fwd ? H : 2 * H, H, rows, G(pre + "mlp.gate_up_proj.weight"), s, nullptr, true, nullptr, false, f16fwd ? 3 : -1));
    } else {
      FV_TRY(dgrad(h, tp, ws, dx, H, H, Tw.downT, I, rows, dtmp, s, nullptr, Tw.downT16));  // d act [rows][I]
      FV_TRY(wgrad(h, tp, ws, dx, H, H, ACT(l), I2, I, rows, G(pre + "mlp.down_proj.weight"), s));   // the kept activation's hi half is the operand
      // d gate/up straight into the split-bf16 form both of its consumers read (no fp32 copy, no separate split pass)
      FV_P(FV_FAM_ELT, 16.0 * rows * I, 20.0 * rows * I, fv::launch_swiglu_bwd(GU(l), dtmp, rows, I, s, dsplit));
      // gate/up: gu = xn2 . Wgu^T
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, I2, Tw.guT, H, rows, dtmp, s, dsplit, Tw.guT16)); // d xn2 [rows][H]
      FV_TRY(wgrad(h, tp, ws, nullptr, 0, I2, XN2(l), 2 * H, H, rows, G(pre + "mlp.gate_up_proj.weight"), s, dsplit));
    }
    FV_P(FV_FAM_NORM, 12.0 * rows * H, 20.0 * rows * H,
         fv::launch_rmsnorm_bwd(X_mid(l), Lw.ln2, dtmp, dx, dx, G(pre + "post_attention_layernorm.weight"), scr, rows, H, d.rms_eps, s));
    // o projection: x_mid = x_in + att . Wo^T
    if (direct) {
      FV_P(FV_FAM_ELT, 0.0, (double)rows * H * 6, fv::launch_rows_to_f16(dx, 0, H, 0, dsplit, H, rows, H, h->f16_flags, s));
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, H, Tw.oT, qd, rows, dtmp, s, nullptr, Tw.oT16, dsplit));   // d att [rows][qd]
      FV_TRY(lora_direct_call(h, l, 1, dsplit, ATT(l), 2, 2 * qd, qd, rows, lora_params, lora_grads, s));
    } else if (fp16_backward(h)) {
      FV_TRY(grad_operands(h, tp, ws, dx, H, H, rows, reinterpret_cast<bf16_t*>(ws + tp.AT), s));
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, H, Tw.oT, qd, rows, dtmp, s, nullptr, Tw.oT16, dsplit));   // d att [rows][qd]
      FV_TRY(wgrad(h, tp, ws, nullptr, 0, H, ATT(l), 2 * qd, qd, rows, G(pre + "self_attn.o_proj.weight"), s, nullptr, true));
    } else {
      FV_TRY(dgrad(h, tp, ws, dx, H, H, Tw.oT, qd, rows, dtmp, s, nullptr, Tw.oT16));       // d att [rows][qd]
      FV_TRY(wgrad(h, tp, ws, dx, H, H, ATT(l), 2 * qd, qd, rows, G(pre + "self_attn.o_proj.weight"), s));
    }
    FV_P(FV_FAM_ATTN, 8.0 * B * (double)Tt * Tt * qd, 4.0 * rows * (2 * qkvw + 2 * qd),
         fv::launch_attention_bwd(QKV(l), qkvw, ATT(l), ATT(l) + qd, 2 * qd, dtmp, qd, LSE(l), delta, dqkv, B, Tt, d.llm_heads, d.llm_kv_heads, D, lens, Ni,
                                  att_scale, h->rope, s, apart, ws + tp.attn_scr));
    if (!direct) FV_TRY(fv::launch_colsum(dqkv, qkvw, rows, qkvw, G(pre + "self_attn.qkv_proj.bias"), colscr, s));
    if (direct) {
      FV_P(FV_FAM_ELT, 0.0, (double)rows * qkvw * 6, fv::launch_rows_to_f16(dqkv, 0, qkvw, 0, dsplit, qkvw, rows, qkvw, h->f16_flags, s));
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, qkvw, Tw.qkvT, H, rows, dtmp, s, nullptr, Tw.qkvT16, dsplit));   // d xn1 [rows][H]
      FV_TRY(lora_direct_call(h, l, 0, dsplit, XN1(l), 2, 2 * H, H, rows, lora_params, lora_grads, s));
    } else if (fp16_backward(h)) {
      FV_TRY(grad_operands(h, tp, ws, dqkv, qkvw, qkvw, rows, reinterpret_cast<bf16_t*>(ws + tp.AT), s));
      FV_TRY(dgrad(h, tp, ws, nullptr, 0, qkvw, Tw.qkvT, H, rows, dtmp, s, nullptr, Tw.qkvT16, dsplit));   // d xn1 [rows][H]
      FV_TRY(wgrad(h, tp, ws, nullptr, 0, qkvw, XN1(l), f16fwd ? H : 2 * H, H, rows, G(pre + "self_attn.qkv_proj.weight"), s, nullptr, true, nullptr, false, f16fwd ? 3 : -1));
    } else {
      FV_TRY(dgrad(h, tp, ws, dqkv, qkvw, qkvw, Tw.qkvT, H, rows, dtmp, s, nullptr, Tw.qkvT16));   // d xn1 [rows][H]
      FV_TRY(wgrad(h, tp, ws, dqkv, qkvw, qkvw, XN1(l), 2 * H, H, rows, G(pre + "self_attn.qkv_proj.weight"), s));
    }
    FV_P(FV_FAM_NORM, 12.0 * rows * H, 20.0 * rows * H,
         fv::launch_rmsnorm_bwd(X_in(l), Lw.ln1, dtmp, dx, dx, G(pre + "input_layernorm.weight"), scr, rows, H, d.rms_eps, s));
    bucket_done(TB_LAYER0 + l);
  }
  // embedding rows of the text positions (direct LoRA: the embedding is frozen and its gradient -- memset and scatter -- is not computed)
  if (!direct) {
    float* gE = G("model.embed_tokens.weight");
    FV_HIP_CHECK(hipMemsetAsync(gE, 0, (size_t)d.llm_vocab * H * 4, s));
    FV_TRY(fv::launch_embed_bwd(ids, lens, dx, gE, B, T, Ni, H, d.llm_vocab, s));
    bucket_done(TB_EMBED);
  }
  // projector: tok = gelu(tower_out . W0^T + b0) . W2^T + b2 at the image positions
  {
    float* dtok = dqkv;   // [RI][H] fp32 (the attention scratch is free now)
    FV_TRY(fv::launch_image_rows(dx, dtok, B, Tt, Ni, H, s));
    FV_TRY(fv::launch_colsum(dtok, H, RI, H, G("model.mm_projector.2.bias"), colscr, s));
    FV_TRY(dgrad(h, tp, ws, dtok, H, H, h->train.pj2T, H, RI, dtmp, s, nullptr, h->train.pj2T16));   // d h [RI][H]
    FV_TRY(wgrad(h, tp, ws, dtok, H, H, hsplit, 2 * H, H, RI, G("model.mm_projector.2.weight"), s));
    FV_TRY(fv::launch_gelu_bwd(dtmp, pre0, (size_t)RI * H, s));
    FV_TRY(fv::launch_colsum(dtmp, H, RI, H, G("model.mm_projector.0.bias"), colscr, s));
    FV_TRY(wgrad(h, tp, ws, dtmp, H, H, tower_out, CO, CO, RI, G("model.mm_projector.0.weight"), s));
    bucket_done(TB_PROJ);
    if (h->train.d_tower_out) {
      // dL/d(tower_out) = d pre0 . W0, straight out as the fp16 rows the tower's backward continues from (fv_train_tower_backward)
      if (!fp16_backward(h)) return fv_fail(FV_ERR_UNSUPPORTED, "tower training runs on the default one-pass fp16 backward (fv_train_set_options 2, 1, k)");
      FV_P(FV_FAM_ELT, 0.0, (double)RI * H * 6, fv::launch_rows_to_f16(dtmp, 0, H, 0, dsplit, H, RI, H, h->f16_flags, s));
      // (fp32 first: the stream gets its own power-of-two scale on the way to fp16 -- tower_bwd_kernels.hip launch_rescale_to_f16; d pre0 in dtmp has been consumed.
      // Its target, twice the loss scale -- 2^13 by default --, follows fv_train_set_options: a caller that lowers the loss scale after fp16 saturations lowers
      // the tower's stream with it)
      fv::GemmArgs g{dsplit, H, h->train.pj0T16, RI, CO, H, nullptr, nullptr, nullptr, 0, dtmp, CO, FV_EPI_F32, 0};
      g.f16 = 1;
      FV_TRY(gemm_p(h, g, s));
      FV_P(FV_FAM_ELT, 0.0, (double)RI * CO * 10, fv::launch_rescale_to_f16(dtmp, static_cast<bf16_t*>(h->train.d_tower_out), (size_t)RI * CO, std::ldexp(2.0f, h->train.loss_scale_log2),
                                                                              reinterpret_cast<unsigned*>(h->train.tscale + 2), h->train.tscale, h->f16_flags, s));
    }
  }
  return FV_OK;
}

int fv_train_forward_backward(fv_handle* h, const float* flat_params, const void* tower_out, const int32_t* ids, const int32_t* lens,
                              const float* states, const float* targets, int B, int T, int training, float dropout_p, uint64_t seed,
                              uint64_t offset, void* ws, size_t ws_bytes, float* actions, float* loss, float* flat_grads, fv_bucket_cb cb,
                              void* user, fv_stream st) {
  if (h && h->train.ready && !flat_grads) {   // (null flat_grads is the impl's switch to the direct LoRA backward: not through this entry point)
    HandleScope _hs(h);
    return fv_fail(FV_ERR_ARG, "fv_train_forward_backward: null pointer");
  }
  return train_forward_backward_impl(h, flat_params, tower_out, ids, lens, states, targets, B, T, training, dropout_p, seed, offset, ws, ws_bytes, actions, loss,
                                     flat_grads, cb, user, st, nullptr, nullptr);
}

}  // extern "C"
