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
//
// Structure.  train_tensors is the one list of what trains (offset, bucket and, for the decoder's own tensors, layer and role: nothing downstream reads a name).
// The step (train_forward_backward_impl) builds ONE DecCtx -- plan, workspace, stream, the backward's mode decided once, every gradient pointer and bucket range
// from one pass over that list -- and runs fwd_gemm (a forward projection in the form f16fwd selects), mlp_backward and proj_backward (the only places that
// switch on the mode) over it.  dgrad / wgrad take the gradient as a GradOp and the activation as an ActOp: values that NAME the form the operand exists in.

namespace {

// what a tensor of the decoder / projector is (TrainTensor::role): the seven of a layer, then the named ones outside the layers
enum { DR_LN1, DR_QKV_W, DR_QKV_B, DR_O_W, DR_LN2, DR_GU_W, DR_DOWN_W, DR_LAYER_ROLES,
       DR_PJ0_W = DR_LAYER_ROLES, DR_PJ0_B, DR_PJ2_W, DR_PJ2_B, DR_EMBED, DR_NORM, DR_ROLES };

struct TrainTensor {
  std::string name;
  int64_t off = 0, numel = 0;
  int rows = 1, cols = 0, bucket = 0, packing = 0;
  int layer = -1, role = -1;   // decoder layer and DR_* role; -1: outside the layers / none (head, tower, adapters)
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

std::vector<TrainTensor> train_tensors(fv_handle* h, int64_t* total) {
  const fv_model_desc& d = h->d;
  std::vector<TrainTensor> out;
  int64_t off = 0;
  int layer = -1;
  auto add = [&](int role, const std::string& n, int rows, int cols, int bucket, void* lib, bool mat, int packing = 0, bf16_t** tc = nullptr, bf16_t** tc16 = nullptr) {
    TrainTensor t;
    t.name = n; t.layer = layer; t.role = role; t.off = off; t.rows = rows; t.cols = cols; t.numel = (int64_t)rows * cols; t.bucket = bucket; t.lib = lib; t.is_mat = mat;
    t.packing = packing; t.tcopy = tc; t.tcopy16 = tc16;
    off += (t.numel + 3) / 4 * 4;
    out.push_back(t);
  };
  static const char* head_names[12] = {"state_projection.0.weight", "state_projection.0.bias", "state_projection.1.weight", "state_projection.1.bias",
                                       "fusion.0.weight", "fusion.0.bias", "fusion.1.weight", "fusion.1.bias", "fusion.4.weight", "fusion.4.bias",
                                       "action_head.weight", "action_head.bias"};
  const fv::HeadOffsets ho = fv::head_offsets(h->hd);
  const fv::HeadDims& hd = h->hd;
  const int hrows[12] = {1, 1, hd.hid, 1, hd.fus, 1, 1, 1, hd.fus, 1, fv::head_out_width(hd), 1};
  const int hcols[12] = {hd.ds, hd.ds, hd.ds, hd.hid, fv::head_cat_width(hd), hd.fus, hd.fus, hd.fus, hd.fus, hd.fus, hd.fus, fv::head_out_width(hd)};
  for (int i = 0; i < 12; ++i) {
    TrainTensor t;
    t.name = head_names[i]; t.off = ho.o[i]; t.rows = hrows[i]; t.cols = hcols[i]; t.numel = (int64_t)t.rows * t.cols; t.bucket = TB_HEAD;
    out.push_back(t);
  }
  off = (ho.o[fv::HP_TOTAL] + 3) / 4 * 4;
  const int H = d.llm_hidden, CO = d.tower_out_dim, I = d.llm_inter, D = d.llm_head_dim;
  const int qd = d.llm_heads * D, kd = d.llm_kv_heads * D, qkvw = qd + 2 * kd;
  Tower& tw = h->tw;
  add(DR_PJ0_W, "model.mm_projector.0.weight", H, CO, TB_PROJ, tw.pj0_w, true, 0, h->train.tower ? &h->train.pj0T : nullptr, h->train.tower ? &h->train.pj0T16 : nullptr);
  add(DR_PJ0_B, "model.mm_projector.0.bias", 1, H, TB_PROJ, tw.pj0_b, false);
  add(DR_PJ2_W, "model.mm_projector.2.weight", H, H, TB_PROJ, tw.pj2_w, true, 0, &h->train.pj2T, &h->train.pj2T16);
  add(DR_PJ2_B, "model.mm_projector.2.bias", 1, H, TB_PROJ, tw.pj2_b, false);
  add(DR_EMBED, "model.embed_tokens.weight", d.llm_vocab, H, TB_EMBED, h->dec.embed, true);
  for (size_t l = 0; l < h->dec.layers.size(); ++l) {
    DecLayer& L = h->dec.layers[l];
    const std::string pre = "model.layers." + std::to_string(l) + ".";
    const int b = TB_LAYER0 + (int)l;
    layer = (int)l;
    TrainLayerT* T = h->train.layers.size() > l ? &h->train.layers[l] : nullptr;
    add(DR_LN1, pre + "input_layernorm.weight", 1, H, b, L.ln1, false);
    add(DR_QKV_W, pre + "self_attn.qkv_proj.weight", qkvw, H, b, L.qkv_w, true, 1, T ? &T->qkvT : nullptr, T ? &T->qkvT16 : nullptr);   // rows: q | k | v
    if (T) out.back().row16 = &T->qkv16;
    add(DR_QKV_B, pre + "self_attn.qkv_proj.bias", 1, qkvw, b, L.qkv_b, false, 1);
    add(DR_O_W, pre + "self_attn.o_proj.weight", H, qd, b, L.o_w, true, 0, T ? &T->oT : nullptr, T ? &T->oT16 : nullptr);
    if (T) out.back().row16 = &T->o16;
    add(DR_LN2, pre + "post_attention_layernorm.weight", 1, H, b, L.ln2, false);
    add(DR_GU_W, pre + "mlp.gate_up_proj.weight", 2 * I, H, b, L.gu_w, true, 2, T ? &T->guT : nullptr, T ? &T->guT16 : nullptr);      // rows: [8 gate | 8 up] blocks
    if (T) out.back().row16 = &T->gu16;
    add(DR_DOWN_W, pre + "mlp.down_proj.weight", H, I, b, L.down_w, true, 0, T ? &T->downT : nullptr, T ? &T->downT16 : nullptr);
    if (T) { out.back().row16 = &T->down16; out.back().scale16 = 16.0f; }
  }
  layer = -1;
  add(DR_NORM, "model.norm.weight", 1, H, TB_LAYER0 + (int)h->dec.layers.size(), h->dec.norm, false);
  if (h->train.tower) append_tower_tensors(h, out, off);
  if (total) *total = off;
  return out;
}

struct TrainPlan {
  int B, T, Ni, Tt, rows, Rp, RI, RIp;
  size_t x_in, x_mid, xn1, qkvf, att, lse, xn2, gu, act;    // per-layer stashes: offset of layer 0, strides below
  size_t s_x, s_xn, s_qkvf, s_att, s_lse, s_gu, s_act, apart;
  size_t pre0, hsplit, tok;                                   // projector stash
  size_t act_s, dx, dtmp, dsplit, AT, XT, dqkv, attn_scr, delta, scr, pooled, dpooled, xg, dxg, head_saved, head_scr, flow_u, flow_act, splitk;
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
  p.flow_u = take(h->hd.te > 0 ? (size_t)fv::head_rows(h->hd, B) * h->hd.da * 4 : 0);   // flow mode: the velocity target u = eps - a of the step (nothing otherwise: the plan keeps its offsets)
  // draws (fv_head_set_flow_draws): the predicted velocity of all S B head rows; the caller's (B, da) `actions` gets draw 0's rows (nothing otherwise)
  p.flow_act = take(fv::head_rows(h->hd, B) > B ? (size_t)fv::head_rows(h->hd, B) * h->hd.da * 4 : 0);
  // split-K partial sums: up to 4 K ranges of the widest fp32 output cut that way (rows x pad(max(H, qkvw)) forward / dgrad, a weight
  // gradient [<= 2I][<= pad(I)] backward); launch_gemm takes as many ranges as fit
  p.splitk_bytes = (size_t)4 * std::max(rows * ((std::max(H, qkvw) + 255) / 256 * 256), std::max(H, qkvw) * ((I + 255) / 256 * 256)) * 4;
  p.splitk = take(p.splitk_bytes);
  p.total = o;
  return p;
}

// one-pass fp16 arithmetic on both sides of the backward (the default options)
bool fp16_backward(const fv_handle* h) { return h->train.grad_split == 2 && h->train.wgrad_f16; }

// how the backward's contractions get their operands.  SPLIT: every dgrad / wgrad makes its own from the fp32 gradient, in the form fv_train_set_options names (the
// split-bf16 forms and every mixed setting); FP16 (the default options): a gradient's fp16 rows and columns from ONE read, shared by its dgrad and its wgrad;
// DIRECT: the direct LoRA backward on top of FP16's options -- fp16 rows only, lora_direct_call in place of every weight-gradient GEMM of the decoder
enum BwdMode { BWD_SPLIT, BWD_FP16, BWD_DIRECT };

struct DecCtx {   // everything one forward / backward step of the decoder needs (after tower_train.inc's TowerCtx); built once per call, never kept
  fv_handle* h; TrainPlan tp; char* ws; hipStream_t s;
  BwdMode mode; bool f16fwd;
  const float* lora_params; float* lora_grads;   // DIRECT: the trainable buffer and its gradient
  fv_bucket_cb cb; void* user;
  std::vector<float*> lgrad;     // [layer][DR_LAYER_ROLES]: where each gradient goes; DIRECT: null behind the projector (no gradient is formed there)
  float* ngrad[DR_ROLES];        // ... and the named tensors outside the layers
  struct Span { int64_t lo = INT64_MAX, hi = 0; };
  std::vector<Span> span;        // [bucket]: its floats [lo, hi) in the gradient buffer
  template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
  // layer l's kept tensors: the residual stream into the layer and between its halves, the normed rows, qkv / lse / attention output, gate/up accumulators, act
  float* X_in(int l) const { return at<float>(tp.x_in + tp.s_x * l); }      float* X_mid(int l) const { return at<float>(tp.x_mid + tp.s_x * l); }
  bf16_t* XN1(int l) const { return at<bf16_t>(tp.xn1 + tp.s_xn * l); }     bf16_t* XN2(int l) const { return at<bf16_t>(tp.xn2 + tp.s_xn * l); }
  float* QKV(int l) const { return at<float>(tp.qkvf + tp.s_qkvf * l); }    float* LSE(int l) const { return at<float>(tp.lse + tp.s_lse * l); }
  bf16_t* ATT(int l) const { return at<bf16_t>(tp.att + tp.s_att * l); }    bf16_t* ACT(int l) const { return at<bf16_t>(tp.act + tp.s_act * l); }
  float* GU(int l) const { return at<float>(tp.gu + tp.s_gu * l); }
  // the backward's scratch: the residual-gradient stream, every dgrad's output, a gradient's 16-bit rows / its columns, an activation's columns
  float* dx() const { return at<float>(tp.dx); }                            float* dtmp() const { return at<float>(tp.dtmp); }
  bf16_t* dsplit() const { return at<bf16_t>(tp.dsplit); }                  bf16_t* AT() const { return at<bf16_t>(tp.AT); }
  bf16_t* XT() const { return at<bf16_t>(tp.XT); }                          float* scr() const { return at<float>(tp.scr); }
  float* colscr() const { return scr() + fv::rmsnorm_bwd_scratch_floats(tp.rows, h->d.llm_hidden); }
  float* G(int l, int role) const { return lgrad[(size_t)l * DR_LAYER_ROLES + role]; }
  float* G(int role) const { return ngrad[role]; }
  void bucket_done(int b) const { if (cb) cb(user, b, span[b].lo, span[b].hi - span[b].lo); }
};

// gbuf: where the head's and the projector's gradients go (and, outside DIRECT, everything else): the full and the trainable layout share that front
DecCtx dec_ctx(fv_handle* h, const TrainPlan& tp, void* ws, hipStream_t s, float* gbuf, const float* lora_params, float* lora_grads, fv_bucket_cb cb, void* user) {
  DecCtx c{h, tp, static_cast<char*>(ws), s, lora_grads ? BWD_DIRECT : (fp16_backward(h) ? BWD_FP16 : BWD_SPLIT), h->train.fwd_f16, lora_params, lora_grads, cb, user};
  c.lgrad.assign(h->dec.layers.size() * DR_LAYER_ROLES, nullptr);
  for (const TrainTensor& t : train_tensors(h, nullptr)) {
    float* g = (c.mode == BWD_DIRECT && t.bucket > TB_PROJ) ? nullptr : gbuf + t.off;
    if (t.layer >= 0) c.lgrad[(size_t)t.layer * DR_LAYER_ROLES + t.role] = g;
    else if (t.role >= 0) c.ngrad[t.role] = g;
    if (c.span.size() <= (size_t)t.bucket) c.span.resize(t.bucket + 1);
    DecCtx::Span& sp = c.span[t.bucket];
    sp.lo = std::min(sp.lo, t.off); sp.hi = std::max(sp.hi, t.off + (t.numel + 3) / 4 * 4);
  }
  c.span[TB_HEAD] = {0, (fv::head_offsets(h->hd).o[fv::HP_TOTAL] + 3) / 4 * 4};   // the head's own layout (and its padding)
  return c;
}

// ---- the operand forms: what a dgrad / wgrad is handed says which copy of its operand EXISTS; the helper makes the one its arithmetic reads ----------------
struct GradOp {   // the gradient dY [R][N]
  enum Form { ROWS_F32, ROWS_SPLIT, ROWS_F16, COLS_F16 } form;
  const float* f32; const bf16_t* p16; int ld;
  static GradOp rows_f32(const float* p, int ld) { return {ROWS_F32, p, nullptr, ld}; }
  static GradOp rows_split(const bf16_t* p) { return {ROWS_SPLIT, nullptr, p, 0}; }   // split bf16 [R][2N] = [hi | lo]
  static GradOp rows_f16(const bf16_t* p) { return {ROWS_F16, nullptr, p, 0}; }       // fp16 rows [R][N], already made (dgrad)
  static GradOp cols_f16(const bf16_t* at) { return {COLS_F16, nullptr, at, 0}; }     // fp16 columns [N][Rp], already in the AT scratch at `at` (wgrad)
};
struct ActOp {    // the activation X [R][K] a weight gradient contracts with
  enum Kind { BF16 = 1, SPLIT = 2, F16 = 3, IN_XT = 4 } kind;   // 1 .. 3: launch_transpose_to_f16's in_kind
  const bf16_t* p; int ld;
  static ActOp bf16(const bf16_t* p, int ld) { return {BF16, p, ld}; }
  static ActOp split(const bf16_t* p, int ld) { return {SPLIT, p, ld}; }   // [hi | lo], the lo half K columns in (the bf16 forms contract with the hi half alone)
  static ActOp f16(const bf16_t* p, int ld) { return {F16, p, ld}; }       // fp16 rows
  static ActOp in_xt() { return {IN_XT, nullptr, 0}; }                     // its fp16 columns sit in the XT scratch already
};
int lora_direct_call(const DecCtx& c, int l, int which, const bf16_t* dY16, const ActOp& X, int R);   // lora_path.inc
int bad_operand(const char* who) { return fv_fail(FV_ERR_STATE, "%s: operand form not available under these backward options (internal)", who); }

int gemm_sk(const DecCtx& c, fv::GemmArgs g) {   // with the split-K scratch attached (few output tiles over a long contraction: launch_gemm cuts along K)
  g.splitk_ws = c.tp.splitk_bytes ? c.at<float>(c.tp.splitk) : nullptr;
  g.splitk_bytes = c.tp.splitk_bytes;
  return gemm_p(c.h, g, c.s);
}

// dW[N][K] (fp32, into the flat gradient) = dY^T . X over `R` rows; both operands transposed into the AT / XT scratch first, unless they are there already
int wgrad(const DecCtx& c, const GradOp& dY, int N, const ActOp& X, int K, int R, float* dW) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const int Rp = (R + 63) / 64 * 64;
  const int sp = h->train.grad_split;   // 0: the gradient's bf16 hi half alone (one pass)
  bf16_t* AT = dY.form == GradOp::COLS_F16 ? const_cast<bf16_t*>(dY.p16) : c.AT();
  bf16_t* XT = c.XT();
  if (h->train.wgrad_f16) {
    // ONE fp16 pass: the (loss-scaled) gradient and the activation both rounded ONCE to 11 significant bits -- 2e-4 per tensor where the
    // split-bf16 gradient against the bf16 (8-bit) activation gave 1.8e-3, at half the MFMA work.  X: the split operand's halves summed first.
    if (dY.form == GradOp::ROWS_SPLIT) FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_transpose_to_f16(dY.p16, 2, 2 * N, N, AT, Rp, R, Rp, N, h->f16_flags, s));
    else if (dY.form == GradOp::ROWS_F32) FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_transpose_to_f16(dY.f32, 0, dY.ld, 0, AT, Rp, R, Rp, N, h->f16_flags, s));
    else if (dY.form != GradOp::COLS_F16) return bad_operand("wgrad");
    if (X.kind != ActOp::IN_XT) FV_P(FV_FAM_ELT, 0.0, (double)R * K * 6, fv::launch_transpose_to_f16(X.p, X.kind, X.ld, K, XT, Rp, R, Rp, K, h->f16_flags, s));
    fv::GemmArgs g16{AT, Rp, XT, N, K, Rp, nullptr, nullptr, nullptr, 0, dW, K, FV_EPI_F32, 0};
    g16.f16 = 1;
    return gemm_sk(c, g16);
  }
  if (X.kind != ActOp::BF16 && X.kind != ActOp::SPLIT) return bad_operand("wgrad");
  if (dY.form != GradOp::ROWS_SPLIT && dY.form != GradOp::ROWS_F32) return bad_operand("wgrad");
  if (dY.form == GradOp::ROWS_SPLIT) {   // its two halves are transposed on their own
    FV_P(FV_FAM_ELT, 0.0, (double)R * N * 4, fv::launch_transpose_to_bf16(dY.p16, 1, 2 * N, AT, 2 * Rp, 0, R, Rp, N, s));
    if (sp) FV_P(FV_FAM_ELT, 0.0, (double)R * N * 4, fv::launch_transpose_to_bf16(dY.p16 + N, 1, 2 * N, AT + Rp, 2 * Rp, 0, R, Rp, N, s));
  } else FV_P(FV_FAM_ELT, 0.0, (double)R * N * 8, fv::launch_transpose_to_bf16(dY.f32, 0, dY.ld, AT, 2 * Rp, sp ? Rp : 0, R, Rp, N, s));
  FV_P(FV_FAM_ELT, 0.0, (double)R * K * 4, fv::launch_transpose_to_bf16(X.p, 1, X.ld, XT, Rp, 0, R, Rp, K, s));
  // few output tiles over a contraction as long as the batch (o_proj: 4 x 4 tiles, K = 2 x 10240): cut along K, one unit per CU
  return gemm_sk(c, fv::GemmArgs{AT, 2 * Rp, XT, N, K, Rp, nullptr, nullptr, nullptr, 0, dW, K, FV_EPI_F32, sp});
}

// dX[R][K] (fp32) = dY[R][N] . W[N][K] through the transposed weight copy: WT [K][N] bf16, WT16 its fp16 twin
int dgrad(const DecCtx& c, const GradOp& dY, int N, const bf16_t* WT, const bf16_t* WT16, int K, int R, float* dX) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const int sp = h->train.grad_split;
  if (sp == 2) {   // ONE fp16 pass: the (loss-scaled) gradient rounded once to 11 bits against the fp16 copy of the transposed weight (exact: bf16 widens into fp16)
    bf16_t* dst = c.dsplit() + (dY.form == GradOp::ROWS_SPLIT ? (size_t)R * 2 * N : 0);   // (a pre-split operand lives in the same scratch: the fp16 rows go behind it)
    if (dY.form == GradOp::ROWS_SPLIT) FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_rows_to_f16(dY.p16, 2, 2 * N, N, dst, N, R, N, h->f16_flags, s));
    else if (dY.form == GradOp::ROWS_F32) FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_rows_to_f16(dY.f32, 0, dY.ld, 0, dst, N, R, N, h->f16_flags, s));
    else if (dY.form != GradOp::ROWS_F16) return bad_operand("dgrad");
    fv::GemmArgs g16{dY.form == GradOp::ROWS_F16 ? dY.p16 : dst, N, WT16, R, K, N, nullptr, nullptr, nullptr, 0, dX, K, FV_EPI_F32, 0};
    g16.f16 = 1;
    return gemm_sk(c, g16);
  }
  const bf16_t* ds = dY.p16;
  if (dY.form == GradOp::ROWS_F32) {
    FV_P(FV_FAM_ELT, 0.0, (double)R * N * 8, fv::launch_split_rows(dY.f32, dY.ld, c.dsplit(), 2 * N, sp ? N : 0, R, N, s));
    ds = c.dsplit();
  } else if (dY.form != GradOp::ROWS_SPLIT) return bad_operand("dgrad");
  return gemm_sk(c, fv::GemmArgs{ds, 2 * N, WT, R, K, N, nullptr, nullptr, nullptr, 0, dX, K, FV_EPI_F32, sp});
}

// FP16: an fp32 gradient's dgrad operand (fp16 rows, in the dsplit scratch) and wgrad operand (fp16 columns, at `at`) from ONE read of it
int grad_operands(const DecCtx& c, const float* dY, int N, int R, bf16_t* at) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const int Rp = (R + 63) / 64 * 64;
  FV_P(FV_FAM_ELT, 0.0, (double)R * N * 8, fv::launch_transpose_to_f16(dY, 0, N, 0, at, Rp, R, Rp, N, h->f16_flags, s, c.dsplit(), N));
  return FV_OK;
}

// host table -> device (the handle owns the allocation)
template <typename T> int upload(fv_handle* h, const std::vector<T>& v, T** dev) {
  void* p = nullptr;
  FV_TRY(dev_alloc(h, v.size() * sizeof(T), &p));
  FV_HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *dev = static_cast<T*>(p);
  return FV_OK;
}

// what one commit launch writes for tensor t (every operand copy the library keeps of it) and how many tiles that takes; tile0 is the table builder's to number
int commit_desc_of(fv_handle* h, const TrainTensor& t, fv::CommitDesc& c, int& ntiles) {
  c = fv::CommitDesc{};
  c.src_off = t.off; c.dst = t.lib; c.is_mat = t.is_mat ? 1 : 0;
  if (t.is_mat) {
    if (t.cols % 8 || t.rows % 8) return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_begin: %s is %d x %d (dimensions must be multiples of 8)", t.name.c_str(), t.rows, t.cols);
    c.rows = t.rows; c.cols = t.cols;
    c.dstT16 = t.tcopy16 ? *t.tcopy16 : nullptr; c.dstTb = t.tcopy ? *t.tcopy : nullptr;
    c.dst16 = (h->train.fwd_f16 && t.row16) ? *t.row16 : nullptr; c.scale16 = t.scale16;
    ntiles = ((t.rows + 63) / 64) * ((t.cols + 63) / 64);
  } else {
    c.rows = 1; c.cols = (int)t.numel;
    ntiles = (int)((t.numel + 4095) / 4096);
  }
  return FV_OK;
}

// fv_train_commit's descriptor table: one launch refreshes every operand copy of the decoder / projector from the master
int build_commit_table(fv_handle* h) {
  std::vector<fv::CommitDesc> cd;
  int tiles = 0;
  for (const TrainTensor& t : train_tensors(h, nullptr)) {
    if (!t.lib) continue;
    fv::CommitDesc c;
    int n = 0;
    FV_TRY(commit_desc_of(h, t, c, n));
    c.tile0 = tiles; tiles += n;
    cd.push_back(c);
  }
  FV_TRY(upload(h, cd, &h->train.commit_desc));
  h->train.commit_n = (int)cd.size(); h->train.commit_tiles = tiles;
  if (h->train.lora.on) FV_TRY(build_lora_tables(h));
  return FV_OK;
}

// fv_train_layout / fv_train_lora_layout: the tensor list as the ABI's records
int write_layout(const char* who, const std::vector<TrainTensor>& tt, fv_train_tensor* out, int max_tensors) {
  if (!out) return FV_OK;
  if (max_tensors < (int)tt.size()) return fv_fail(FV_ERR_ARG, "%s: room for %d tensors, %zu needed", who, max_tensors, tt.size());
  for (size_t i = 0; i < tt.size(); ++i) {
    memset(&out[i], 0, sizeof(out[i]));
    snprintf(out[i].name, sizeof(out[i].name), "%s", tt[i].name.c_str());
    out[i].offset = tt[i].off; out[i].numel = tt[i].numel; out[i].rows = tt[i].rows; out[i].cols = tt[i].cols;
    out[i].bucket = tt[i].bucket; out[i].packing = tt[i].packing;
  }
  return FV_OK;
}

// ---- the step's per-projection pieces --------------------------------------------------------------------------------------------------------
// The training forward's projections come in two forms.  Default: split-bf16 rows [hi | lo] against the bf16 weight (two passes).  f16fwd (fv_train_set_forward_f16):
// ONE fp16 pass -- the normed rows leave the RMSNorm as fp16, the attention output is rounded once from its split form, the SwiGLU output leaves the gate/up epilogue
// as fp16 (x 2^-4, the down copy carries the 2^4); weights = exact fp16 copies of the bf16 weights.  The accumulators the backward differentiates (qkv fp32, gate/up
// stash, lse) and the fp32 residual stream are kept exactly the same in both.
int fwd_norm(const DecCtx& c, const float* x, const float* w, bf16_t* y) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const int H = h->d.llm_hidden, rows = c.tp.rows, f = c.f16fwd ? 1 : 0;
  FV_P(FV_FAM_NORM, 4.0 * rows * H, (f ? 6.0 : 8.0) * rows * H,
       fv::launch_rmsnorm(x, w, y, f ? nullptr : y + H, f ? H : 2 * H, rows, H, h->d.rms_eps, s, f, f ? h->f16_flags : nullptr));
  return FV_OK;
}
// y [rows][N] = x . W^T over K columns (+ res, an fp32 residual [rows][H]): operand, leading dimension and weight copy as f16fwd says
fv::GemmArgs fwd_gemm(const DecCtx& c, const bf16_t* X, const bf16_t* W, const bf16_t* W16, int N, int K, const float* bias, const float* res, void* out, int ldo, int epi) {
  fv::GemmArgs g{X, c.f16fwd ? K : 2 * K, c.f16fwd ? W16 : W, c.tp.rows, N, K, bias, nullptr, res, res ? c.h->d.llm_hidden : 0, out, ldo, epi, c.f16fwd ? 0 : 1};
  g.f16 = c.f16fwd ? 1 : 0;
  return g;
}

// backward of one projection y = x . W^T of layer l (`which`: 0 q|k|v, 1 o -- lora_direct_call's numbering): gradient operands, dX = dY . W, then dW = dY^T . X or,
// DIRECT, dA / dB of the adapters inside W.  THE place the mode is switched on for these two (the MLP pair has its own, below)
int proj_backward(const DecCtx& c, int l, int which, const float* dY, int N, const ActOp& X, int K, const bf16_t* WT, const bf16_t* WT16, float* dX, float* dW) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const int R = c.tp.rows;
  switch (c.mode) {
    case BWD_DIRECT:   // gradient ROWS only (no column copies: nothing here runs a weight-gradient GEMM)
      FV_P(FV_FAM_ELT, 0.0, (double)R * N * 6, fv::launch_rows_to_f16(dY, 0, N, 0, c.dsplit(), N, R, N, h->f16_flags, s));
      FV_TRY(dgrad(c, GradOp::rows_f16(c.dsplit()), N, WT, WT16, K, R, dX));
      return lora_direct_call(c, l, which, c.dsplit(), X, R);
    case BWD_FP16:
      FV_TRY(grad_operands(c, dY, N, R, c.AT()));
      FV_TRY(dgrad(c, GradOp::rows_f16(c.dsplit()), N, WT, WT16, K, R, dX));
      return wgrad(c, GradOp::cols_f16(c.AT()), N, X, K, R, dW);
    case BWD_SPLIT:
      FV_TRY(dgrad(c, GradOp::rows_f32(dY, N), N, WT, WT16, K, R, dX));
      return wgrad(c, GradOp::rows_f32(dY, N), N, X, K, R, dW);
  }
  return FV_OK;
}

// backward of layer l's MLP, x_out = x_mid + act . Wd^T with act = silu(gate) * up, gate/up = xn2 . Wgu^T: dx -> d xn2 in dtmp, dWd, dWgu.  The two projections are
// entangled through the SwiGLU backward, which writes d gate/up (and, FP16 / DIRECT, act) straight into the operand forms its consumers read: once per mode
int mlp_backward(const DecCtx& c, int l) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const TrainLayerT& Tw = h->train.layers[l];
  const int H = h->d.llm_hidden, I = h->d.llm_inter, I2 = 2 * I, rows = c.tp.rows;
  float *dx = c.dx(), *dtmp = c.dtmp();
  bf16_t* dsplit = c.dsplit();
  const ActOp xn2 = c.f16fwd ? ActOp::f16(c.XN2(l), H) : ActOp::split(c.XN2(l), 2 * H);
  switch (c.mode) {
    case BWD_DIRECT: {
      // gradient ROWS only (no column copies: nothing here runs a weight-gradient GEMM).  dx's fp16 rows go into the last third of the dsplit scratch, so that they
      // outlive the SwiGLU backward, which writes d gate/up's rows at its start and silu(gate) * up as fp16 rows (the down adapters' activation) into the XT scratch
      bf16_t* dx16 = dsplit + (size_t)rows * 2 * c.tp.wmax;
      bf16_t* act16 = c.XT();
      FV_P(FV_FAM_ELT, 0.0, (double)rows * H * 6, fv::launch_rows_to_f16(dx, 0, H, 0, dx16, H, rows, H, h->f16_flags, s));
      FV_TRY(dgrad(c, GradOp::rows_f16(dx16), H, Tw.downT, Tw.downT16, I, rows, dtmp));  // d act [rows][I]
      FV_P(FV_FAM_ELT, 18.0 * rows * I, 16.0 * rows * I, fv::launch_swiglu_bwd_rows(c.GU(l), 1, dtmp, rows, rows, I, dsplit, act16, h->f16_flags, s));
      FV_TRY(lora_direct_call(c, l, 3, dx16, ActOp::f16(act16, I), rows));
      FV_TRY(dgrad(c, GradOp::rows_f16(dsplit), I2, Tw.guT, Tw.guT16, H, rows, dtmp)); // d xn2 [rows][H]
      return lora_direct_call(c, l, 2, dsplit, xn2, rows);
    }
    case BWD_FP16: {
      // dx -> fp16 rows + columns in one pass; d act; then the SwiGLU backward writes d gate/up straight into the two fp16 operands its consumers
      // read (rows for the dgrad, columns for the wgrad) AND act^T for the down projection's wgrad, which therefore runs after it
      bf16_t* at0 = c.AT();
      bf16_t* at1 = at0 + (size_t)I2 * c.tp.Rp;   // behind the widest gradient's columns
      FV_TRY(grad_operands(c, dx, H, rows, at1));
      FV_TRY(dgrad(c, GradOp::rows_f16(dsplit), H, Tw.downT, Tw.downT16, I, rows, dtmp));  // d act [rows][I]
      FV_P(FV_FAM_ELT, 18.0 * rows * I, 22.0 * rows * I, fv::launch_swiglu_bwd_f16(c.GU(l), 1, dtmp, rows, c.tp.Rp, I, dsplit, at0, h->f16_flags, s, c.XT()));
      FV_TRY(wgrad(c, GradOp::cols_f16(at1), H, ActOp::in_xt(), I, rows, c.G(l, DR_DOWN_W)));
      FV_TRY(dgrad(c, GradOp::rows_f16(dsplit), I2, Tw.guT, Tw.guT16, H, rows, dtmp)); // d xn2 [rows][H]
      return wgrad(c, GradOp::cols_f16(at0), I2, xn2, H, rows, c.G(l, DR_GU_W));
    }
    case BWD_SPLIT:
      FV_TRY(dgrad(c, GradOp::rows_f32(dx, H), H, Tw.downT, Tw.downT16, I, rows, dtmp));  // d act [rows][I]
      FV_TRY(wgrad(c, GradOp::rows_f32(dx, H), H, ActOp::split(c.ACT(l), I2), I, rows, c.G(l, DR_DOWN_W)));   // the kept activation's hi half is the operand
      // d gate/up straight into the split-bf16 form both of its consumers read (no fp32 copy, no separate split pass)
      FV_P(FV_FAM_ELT, 16.0 * rows * I, 20.0 * rows * I, fv::launch_swiglu_bwd(c.GU(l), dtmp, rows, I, s, dsplit));
      FV_TRY(dgrad(c, GradOp::rows_split(dsplit), I2, Tw.guT, Tw.guT16, H, rows, dtmp)); // d xn2 [rows][H]
      return wgrad(c, GradOp::rows_split(dsplit), I2, xn2, H, rows, c.G(l, DR_GU_W));
  }
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
  return write_layout("fv_train_layout", tt, out, max_tensors);
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
  h->train.layers.resize(h->dec.layers.size());
  // transposed copies of the weights as loaded: bf16 (split / plain dgrad) and fp16 (one-pass dgrad; bf16 widens into fp16 exactly)
  for (const TrainTensor& t : train_tensors(h, nullptr)) {
    if (!t.tcopy) continue;
    void* p = nullptr;
    FV_TRY(dev_alloc(h, (size_t)t.numel * 2, &p)); *t.tcopy = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, (size_t)t.numel * 2, &p)); *t.tcopy16 = static_cast<bf16_t*>(p);
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
  FV_TRY(prompt_invalidate(h, s, true));   // the decoder's (and the tower's) operand images change: the literal call's kept result is void
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
  if (h->train.guard) FV_TRY(guard_range_check("fv_train_set_options", h->train.guard->cfg, loss_scale_log2));   // (a bound step guard moves the scale inside its range)
  FV_TRY(prompt_invalidate(h, nullptr, false));
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
int fv_train_set_step_guard(fv_handle* h, fv_step_guard* guard) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (guard) FV_TRY(guard_range_check("fv_train_set_step_guard", guard->cfg, h->train.loss_scale_log2));
  h->train.guard = guard;
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
  FV_TRY(prompt_invalidate(h, nullptr, false));
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
  if (fv::head_rows(h->hd, B) > B && (offset >> 56 & 15))   // (launch_flow_prepare's check, before the backbone's forward is enqueued)
    return fv_fail(FV_ERR_ARG, "%s: bits 56 .. 59 of the offset number the flow head's draws and must be 0 with more than one draw", who);
  // refused HERE, before anything is enqueued or any bucket's all-reduce is launched (launch_embed_bwd runs at the very end of the backward).  The direct LoRA
  // backward computes no embedding gradient, but fv_train_workspace_bytes sizes the workspace for both entry points and admits no larger step: same limit, its own words
  if ((long)B * T > 16384)
    return direct ? fv_fail(FV_ERR_UNSUPPORTED, "%s: %ld text positions per step (fv_train_workspace_bytes admits B * T <= 16384)", who, (long)B * T)
                  : fv_fail(FV_ERR_UNSUPPORTED, "fv_train_forward_backward: %ld text positions per step (the embedding gradient keeps the batch's ids in 64 KB of LDS: B * T <= 16384)", (long)B * T);
  const TrainPlan tp = plan_train(h, B, T);
  if (tp.total > ws_bytes) return fv_fail(FV_ERR_STATE, "training workspace too small (%zu > %zu)", tp.total, ws_bytes);
  if (((uintptr_t)ws_v | (uintptr_t)gbuf | (uintptr_t)flat_params) & 15) return fv_fail(FV_ERR_ARG, "%s: buffers must be 16-byte aligned", who);
  if (tp.Tt > h->rope_rows) return fv_fail(FV_ERR_ARG, "sequence of %d tokens exceeds the RoPE table (%d)", tp.Tt, h->rope_rows);
  hipStream_t s = static_cast<hipStream_t>(st);
  const DecCtx c = dec_ctx(h, tp, ws_v, s, gbuf, lora_params, lora_grads, cb, user);
  const bf16_t* tower_out = static_cast<const bf16_t*>(tower_out_v);
  const int H = d.llm_hidden, I = d.llm_inter, I2 = 2 * I, D = d.llm_head_dim, CO = d.tower_out_dim;
  const int qd = d.llm_heads * D, kd = d.llm_kv_heads * D, qkvw = qd + 2 * kd;
  const int rows = tp.rows, RI = tp.RI, Ni = tp.Ni, Tt = tp.Tt, L = (int)h->dec.layers.size();
  const float att_scale = 1.0f / std::sqrt((float)D);
  float *pre0 = c.at<float>(tp.pre0), *tok = c.at<float>(tp.tok), *pooled = c.at<float>(tp.pooled), *head_saved = c.at<float>(tp.head_saved);
  bf16_t *hsplit = c.at<bf16_t>(tp.hsplit), *dsplit = c.dsplit();
  float *dx = c.dx(), *dtmp = c.dtmp(), *dqkv = c.at<float>(tp.dqkv), *scr = c.scr(), *colscr = c.colscr();
  void* attn_scr = c.at<char>(tp.attn_scr);
  Tower& tw = h->tw;

  // ------------------------------------------------------------------------------------------------ forward (everything kept)
  FV_TRY(gemm_p(h, fv::GemmArgs{tower_out, CO, tw.pj0_w, RI, H, CO, tw.pj0_b, nullptr, nullptr, 0, pre0, H, FV_EPI_F32, 0}, s));
  FV_P(FV_FAM_ELT, 20.0 * RI * H, 8.0 * RI * H, fv::launch_gelu_fwd(pre0, hsplit, 2 * H, H, RI, H, s));
  FV_TRY(gemm_p(h, fv::GemmArgs{hsplit, 2 * H, tw.pj2_w, RI, H, H, tw.pj2_b, nullptr, nullptr, 0, tok, H, FV_EPI_F32, 1}, s));
  FV_P(FV_FAM_ELT, 0.0, 6.0 * rows * H, fv::launch_embed_gather(ids, h->dec.embed, tok, c.X_in(0), B, T, Ni, H, d.llm_vocab, s));
  if (c.f16fwd && c.mode == BWD_SPLIT) return fv_fail(FV_ERR_UNSUPPORTED, "the fp16 training forward goes with the default one-pass fp16 backward (fv_train_set_options 2, 1, k)");
  for (int l = 0; l < L; ++l) {
    const DecLayer& Lw = h->dec.layers[l];
    const TrainLayerT& Tw = h->train.layers[l];
    FV_TRY(fwd_norm(c, c.X_in(l), Lw.ln1, c.XN1(l)));
    FV_TRY(gemm_sk(c, fwd_gemm(c, c.XN1(l), Lw.qkv_w, Tw.qkv16, qkvw, H, Lw.qkv_b, nullptr, c.QKV(l), qkvw, FV_EPI_F32)));
    FV_P(FV_FAM_ATTN, 2.0 * B * (double)Tt * Tt * qd, 4.0 * rows * (qkvw + qd),
         fv::launch_attention_f32(c.QKV(l), qkvw, c.ATT(l), c.ATT(l) + qd, 2 * qd, B, Tt, d.llm_heads, d.llm_kv_heads, D, lens, Ni, att_scale, s, h->rope, nullptr, 0, 0, c.LSE(l), 0, attn_scr));
    const bf16_t* att = c.ATT(l);   // kept split for the backward; the fp16 forward reads it rounded once to fp16 rows
    if (c.f16fwd) {
      FV_P(FV_FAM_ELT, 0.0, (double)rows * qd * 6, fv::launch_rows_to_f16(c.ATT(l), 2, 2 * qd, qd, dsplit, qd, rows, qd, h->f16_flags, s));
      att = dsplit;
    }
    FV_TRY(gemm_sk(c, fwd_gemm(c, att, Lw.o_w, Tw.o16, H, qd, nullptr, c.X_in(l), c.X_mid(l), H, FV_EPI_RES_F32)));
    FV_TRY(fwd_norm(c, c.X_mid(l), Lw.ln2, c.XN2(l)));
    {   // gate/up with the SwiGLU in its epilogue (act leaves as the down projection's operand) AND the raw accumulators kept for the backward
      fv::GemmArgs g1 = fwd_gemm(c, c.XN2(l), Lw.gu_w, Tw.gu16, I2, H, nullptr, nullptr, c.ACT(l), c.f16fwd ? I : I2, c.f16fwd ? FV_EPI_SWIGLU_F16 : FV_EPI_SWIGLU_SPLIT);
      g1.stash = c.GU(l);
      // the one-pass fp16 backward rounds d gate/up and act to fp16 operands anyway: it keeps the accumulators as fp16 too (the epilogue of this
      // launch is write-bound: 600 -> 400 MB; the SwiGLU backward reads 200 MB less)
      g1.stash_f16 = c.mode != BWD_SPLIT ? 1 : 0; g1.sat = h->f16_flags;
      FV_TRY(gemm_p(h, g1, s));
    }
    FV_TRY(gemm_sk(c, fwd_gemm(c, c.ACT(l), Lw.down_w, Tw.down16, H, I, nullptr, c.X_mid(l), c.X_in(l + 1), H, FV_EPI_RES_F32)));
  }
  FV_P(FV_FAM_ELT, 4.0 * B * H, 8.0 * B * H, fv::launch_pool_norm(c.X_in(L), lens, h->dec.norm, pooled, B, Tt, Ni, H, d.rms_eps, 0, s));
  const fv::HeadIoNorm* io = h->has_io ? &h->io : nullptr;
  // flow mode: the one place where the backbone routes noise their targets -- x_t and phi(t) go into head_saved's cat columns from the step's (seed, offset), as
  // fv_head_flow_prepare does for the head-only route, and the loss below compares the predicted velocity with u
  // draws (fv_head_set_flow_draws): the S draws are prepared HERE, once, for every route; the head runs on S B rows into the plan's own predictions (the
  // caller's `actions` gets draw 0's rows), the loss is the S-draw loss, and launch_head_backward hands back d_pooled summed over the draws -- B rows, which
  // the backbone's backward below continues from as it is
  const float* head_targets = targets;
  float* head_actions = fv::head_rows(h->hd, B) > B ? c.at<float>(tp.flow_act) : actions;
  if (h->hd.te > 0) {
    float* u = c.at<float>(tp.flow_u);
    FV_P(FV_FAM_HEAD, 0.0, 0.0, fv::launch_flow_prepare(h->hd, h->flow, targets, B, seed, offset, nullptr, nullptr, head_saved, u, s));
    head_targets = u;
  }
  // training != 0: the loss lives in normalised action space (fv_head_forward's convention)
  FV_P(FV_FAM_HEAD, 0.0, 0.0, fv::launch_head_forward(h->hd, flat_params, pooled, states, B, training ? (dropout_p > 0.f ? 1 : 2) : 2, dropout_p, seed, offset, head_actions,
                                                     head_saved, s, io));
  if (head_actions != actions) FV_HIP_CHECK(hipMemcpyAsync(actions, head_actions, (size_t)B * h->hd.da * 4, hipMemcpyDeviceToDevice, s));

  // ------------------------------------------------------------------------------------------------ backward
  float *dpooled = c.at<float>(tp.dpooled), *xg = c.at<float>(tp.xg), *dxg = c.at<float>(tp.dxg);
  FV_P(FV_FAM_HEAD, 0.0, 0.0, fv::launch_head_backward(h->hd, flat_params, nullptr, head_actions, head_targets, B, dropout_p, head_saved, loss, gbuf, c.at<float>(tp.head_scr), s, dpooled,
                                                      std::ldexp(1.0f, h->train.loss_scale_log2), &h->loss, h->train.guard ? &h->train.guard->w->delta : nullptr));
  c.bucket_done(TB_HEAD);
  // final norm on the pooled rows; the residual-gradient stream starts as zero everywhere else
  FV_TRY(fv::launch_pool_rows(c.X_in(L), xg, lens, B, Tt, Ni, H, 0, s));
  FV_TRY(fv::launch_rmsnorm_bwd(xg, h->dec.norm, dpooled, nullptr, dxg, c.G(DR_NORM), scr, B, H, d.rms_eps, s));
  FV_HIP_CHECK(hipMemsetAsync(dx, 0, (size_t)rows * H * 4, s));
  FV_TRY(fv::launch_pool_rows(dx, dxg, lens, B, Tt, Ni, H, 1, s));
  c.bucket_done(TB_LAYER0 + L);
  for (int l = L - 1; l >= 0; --l) {
    const DecLayer& Lw = h->dec.layers[l];
    const TrainLayerT& Tw = h->train.layers[l];
    FV_TRY(mlp_backward(c, l));   // down, SwiGLU, gate/up: dx -> d xn2 in dtmp
    FV_P(FV_FAM_NORM, 12.0 * rows * H, 20.0 * rows * H, fv::launch_rmsnorm_bwd(c.X_mid(l), Lw.ln2, dtmp, dx, dx, c.G(l, DR_LN2), scr, rows, H, d.rms_eps, s));
    // o projection: x_mid = x_in + att . Wo^T; d att [rows][qd] into dtmp
    FV_TRY(proj_backward(c, l, 1, dx, H, ActOp::split(c.ATT(l), 2 * qd), qd, Tw.oT, Tw.oT16, dtmp, c.G(l, DR_O_W)));
    FV_P(FV_FAM_ATTN, 8.0 * B * (double)Tt * Tt * qd, 4.0 * rows * (2 * qkvw + 2 * qd),
         fv::launch_attention_bwd(c.QKV(l), qkvw, c.ATT(l), c.ATT(l) + qd, 2 * qd, dtmp, qd, c.LSE(l), c.at<float>(tp.delta), dqkv, B, Tt, d.llm_heads, d.llm_kv_heads, D, lens, Ni,
                                  att_scale, h->rope, s, c.at<float>(tp.apart), attn_scr));
    if (c.mode != BWD_DIRECT) FV_TRY(fv::launch_colsum(dqkv, qkvw, rows, qkvw, c.G(l, DR_QKV_B), colscr, s));
    // qkv projection: qkv = xn1 . Wqkv^T + b; d xn1 [rows][H] into dtmp
    FV_TRY(proj_backward(c, l, 0, dqkv, qkvw, c.f16fwd ? ActOp::f16(c.XN1(l), H) : ActOp::split(c.XN1(l), 2 * H), H, Tw.qkvT, Tw.qkvT16, dtmp, c.G(l, DR_QKV_W)));
    FV_P(FV_FAM_NORM, 12.0 * rows * H, 20.0 * rows * H, fv::launch_rmsnorm_bwd(c.X_in(l), Lw.ln1, dtmp, dx, dx, c.G(l, DR_LN1), scr, rows, H, d.rms_eps, s));
    c.bucket_done(TB_LAYER0 + l);
  }
  // embedding rows of the text positions (direct LoRA: the embedding is frozen and its gradient -- memset and scatter -- is not computed)
  if (c.mode != BWD_DIRECT) {
    float* gE = c.G(DR_EMBED);
    FV_HIP_CHECK(hipMemsetAsync(gE, 0, (size_t)d.llm_vocab * H * 4, s));
    FV_TRY(fv::launch_embed_bwd(ids, lens, dx, gE, B, T, Ni, H, d.llm_vocab, s));
    c.bucket_done(TB_EMBED);
  }
  // projector: tok = gelu(tower_out . W0^T + b0) . W2^T + b2 at the image positions (every mode: each helper makes the operand form the options name)
  {
    float* dtok = dqkv;   // [RI][H] fp32 (the attention scratch is free now)
    FV_TRY(fv::launch_image_rows(dx, dtok, B, Tt, Ni, H, s));
    FV_TRY(fv::launch_colsum(dtok, H, RI, H, c.G(DR_PJ2_B), colscr, s));
    FV_TRY(dgrad(c, GradOp::rows_f32(dtok, H), H, h->train.pj2T, h->train.pj2T16, H, RI, dtmp));   // d h [RI][H]
    FV_TRY(wgrad(c, GradOp::rows_f32(dtok, H), H, ActOp::split(hsplit, 2 * H), H, RI, c.G(DR_PJ2_W)));
    FV_TRY(fv::launch_gelu_bwd(dtmp, pre0, (size_t)RI * H, s));
    FV_TRY(fv::launch_colsum(dtmp, H, RI, H, c.G(DR_PJ0_B), colscr, s));
    FV_TRY(wgrad(c, GradOp::rows_f32(dtmp, H), H, ActOp::bf16(tower_out, CO), CO, RI, c.G(DR_PJ0_W)));
    c.bucket_done(TB_PROJ);
    if (h->train.d_tower_out) {
      // dL/d(tower_out) = d pre0 . W0, straight out as the fp16 rows the tower's backward continues from (fv_train_tower_backward)
      if (c.mode == BWD_SPLIT) return fv_fail(FV_ERR_UNSUPPORTED, "tower training runs on the default one-pass fp16 backward (fv_train_set_options 2, 1, k)");
      FV_P(FV_FAM_ELT, 0.0, (double)RI * H * 6, fv::launch_rows_to_f16(dtmp, 0, H, 0, dsplit, H, RI, H, h->f16_flags, s));
      // (fp32 first: the stream gets its own power-of-two scale on the way to fp16 -- tower_bwd_kernels.hip launch_rescale_to_f16; d pre0 in dtmp has been consumed.
      // Its target, twice the loss scale -- 2^13 by default --, follows fv_train_set_options: a caller that lowers the loss scale after fp16 saturations lowers
      // the tower's stream with it)
      fv::GemmArgs g{dsplit, H, h->train.pj0T16, RI, CO, H, nullptr, nullptr, nullptr, 0, dtmp, CO, FV_EPI_F32, 0};
      g.f16 = 1;
      FV_TRY(gemm_p(h, g, s));
      FV_P(FV_FAM_ELT, 0.0, (double)RI * CO * 10, fv::launch_rescale_to_f16(dtmp, static_cast<bf16_t*>(h->train.d_tower_out), (size_t)RI * CO, std::ldexp(2.0f, h->train.loss_scale_log2),
                                                                              reinterpret_cast<unsigned*>(h->train.tscale + 2), h->train.tscale, h->f16_flags, s,
                                                                              h->train.guard ? &h->train.guard->w->delta : nullptr));   // (a bound step guard: the target follows 2^k delta)
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
