// lora_path.inc -- host side of the LoRA mode of backbone training (fv_train_lora_*), included by engine.hip behind train_path.inc.
//
// The reference has no adapter mode: its one knob is fastvla/configuration_fastvla.py:23 `freeze_backbone` and its step body training/trainer.py:60-66,
// 171-182 (clip_grad_norm_ + AdamW over the parameters with requires_grad).  Here the decoder's matrices stay frozen in the fp32 master and every TARGET
// matrix (q, k, v, o, gate, up, down of every layer) runs as W0 + s . B . A, s = alpha / rank -- PEFT's merged LoRA without dropout.  The TRAINABLE
// parameters live in a flat buffer of their own,
//     [ action expert | projector | layer 0 adapters .. layer L-1 adapters ]        (fv_train_lora_layout)
// whose front (head + projector) has the master's own offsets; gradients and Adam's m / v mirror THAT buffer.  One step:
//     fv_train_forward_backward (unchanged: full dW' into the full gradient buffer)  ->  fv_train_lora_project (dA, dB; head / projector gradients copied)
//     ->  all-reduce + fv_adamw_clip_step over the trainable buffer  ->  fv_train_lora_commit (operand images from W0 + s . B . A).
// The DIRECT mode replaces the first two by fv_train_lora_forward_backward: the same forward and dgrad chain (train_path.inc, ONE body), dA / dB of every adapter
// straight from the gradient's fp16 rows and the kept activations (lora_direct_kernels.hip) into the trainable-layout gradient buffer; no full gradient buffer.
// Two variants ride on fv_train_lora_begin_ex's flags.  FV_LORA_RSLORA: s = alpha / sqrt(rank) -- ls.scale, nothing else.  FV_LORA_DORA (PEFT's use_dora): every
// target also owns a magnitude vector m (`out` floats, "...lora_magnitude_vector.weight", behind its lora_B in the trainable buffer) and runs as
// diag(m / n) (W0 + s . B . A), n the row norms, which the commit refreshes into a buffer the handle owns and the projection reads (norm held constant in the
// backward, as PEFT does); the direct backward refuses it.
// Structure.  lora_tensors lays the trainable buffer out and keeps every adapter's offsets by (layer, target, A | B | m).  build_lora_tables makes every device table
// and the direct backward's packs in ONE pass over train_tensors, finding a layer's adapted tensors by TrainTensor::layer / role and building each descriptor with
// train_path.inc's commit_desc_of (so does fv_train_commit's table); the entry points share check_buffers, write_layout and upload.
// Kernels: lora_kernels.hip, lora_direct_kernels.hip.

namespace {

const char* const LORA_TARGET_NAMES[7] = {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"};

// one target of a layer: where it sits inside its packed tensor (that tensor's DR_* role, `which` of lora_direct_call's four, row layout `kind`, `part` within it)
struct LoraLogical { int out, in, row0, blk, role, which, kind, part; };

void lora_logicals(const fv_model_desc& d, LoraLogical out[7]) {
  const int H = d.llm_hidden, I = d.llm_inter, D = d.llm_head_dim, qd = d.llm_heads * D, kd = d.llm_kv_heads * D;
  out[0] = {qd, H, 0, 8, DR_QKV_W, 0, 1, 0};
  out[1] = {kd, H, qd, 8, DR_QKV_W, 0, 1, 1};
  out[2] = {kd, H, qd + kd, 8, DR_QKV_W, 0, 1, 2};
  out[3] = {H, qd, 0, 8, DR_O_W, 1, 0, 0};
  out[4] = {I, H, 0, 16, DR_GU_W, 2, 2, 0};
  out[5] = {I, H, 8, 16, DR_GU_W, 2, 2, 1};
  out[6] = {H, I, 0, 8, DR_DOWN_W, 3, 0, 0};
}

// the trainable buffer: head and projector exactly as train_tensors lists them (same offsets), then lora_A (rank x in) / lora_B (out x rank) [/ DoRA's magnitude,
// one float per output row] per layer and target
struct LoraLayout {
  std::vector<TrainTensor> tensors;
  int64_t total = 0, front = 0;      // floats in all; floats of the head + projector front
  std::vector<int64_t> offs;         // [layer][target][A, B, m]: offset in the trainable buffer, -1 = not there
  int64_t off(int l, int k, int abm) const { return offs[((size_t)l * 7 + k) * 3 + abm]; }
};
LoraLayout lora_tensors(fv_handle* h, int rank, int mask, bool dora) {
  LoraLayout lay;
  int64_t off = 0;
  for (const TrainTensor& t : train_tensors(h, nullptr)) {
    if (t.bucket > TB_PROJ) { off = t.off; break; }
    TrainTensor c = t;
    c.lib = nullptr; c.tcopy = c.tcopy16 = c.row16 = nullptr;
    lay.tensors.push_back(c);
  }
  lay.front = off;
  lay.offs.assign((size_t)h->d.llm_layers * 7 * 3, -1);
  LoraLogical lg[7];
  lora_logicals(h->d, lg);
  static const char* const suffix[3] = {".lora_A.weight", ".lora_B.weight", ".lora_magnitude_vector.weight"};
  for (int l = 0; l < h->d.llm_layers; ++l)
    for (int k = 0; k < 7; ++k) {
      if (!(mask >> k & 1)) continue;
      const std::string pre = "model.layers." + std::to_string(l) + "." + LORA_TARGET_NAMES[k];
      for (int abm = 0; abm < (dora ? 3 : 2); ++abm) {
        TrainTensor t;
        t.name = pre + suffix[abm];
        t.rows = abm == 0 ? rank : (abm == 1 ? lg[k].out : 1); t.cols = abm == 0 ? lg[k].in : (abm == 1 ? rank : lg[k].out); t.numel = (int64_t)t.rows * t.cols;
        t.off = off; t.bucket = TB_LAYER0 + l; t.is_mat = abm < 2;
        lay.offs[((size_t)l * 7 + k) * 3 + abm] = off;
        off += (t.numel + 3) / 4 * 4;
        lay.tensors.push_back(t);
      }
    }
  lay.total = off;
  return lay;
}

// every table the LoRA entry points read, from ONE pass over train_tensors: the adapted matrices, the commit descriptors of the packed tensors that hold them, the
// plain commit table of the rest, and the direct backward's calls (one per packed tensor and layer, the adapters inside it as slots in part order)
int build_lora_tables(fv_handle* h) {
  LoraState& ls = h->train.lora;
  const fv_model_desc& d = h->d;
  const int rank = ls.rank, qd = d.llm_heads * d.llm_head_dim, kd = d.llm_kv_heads * d.llm_head_dim;
  LoraLogical lg[7];
  lora_logicals(d, lg);
  const bool dora = (ls.flags & FV_LORA_DORA) != 0;
  const LoraLayout lay = lora_tensors(h, rank, ls.mask, dora);
  std::vector<fv::LoraMat> mats;
  std::vector<fv::LoraCommitDesc> cds;
  std::vector<fv::CommitDesc> rest;
  std::vector<fv::LoraDirectPack> packs((size_t)d.llm_layers * 4, fv::LoraDirectPack{});
  int ctiles = 0, rtiles = 0, strips = 0, bands = 0;
  long long nrows = 0;
  for (const TrainTensor& t : train_tensors(h, nullptr)) {
    if (!t.lib) continue;
    fv::LoraCommitDesc lc{};
    int ntile = 0;
    FV_TRY(commit_desc_of(h, t, lc.c, ntile));
    lc.mat[0] = lc.mat[1] = lc.mat[2] = -1;
    bool adapted = false;
    for (int k = 0; k < 7 && t.layer >= 0; ++k) {
      if (!(ls.mask >> k & 1) || t.role != lg[k].role) continue;
      const int l = t.layer;
      fv::LoraMat m{};
      m.w_off = t.off; m.out = lg[k].out; m.in = lg[k].in; m.row0 = lg[k].row0; m.blk = lg[k].blk;
      m.a_off = lay.off(l, k, 0); m.b_off = lay.off(l, k, 1); m.m_off = lay.off(l, k, 2);
      if (m.in != t.cols || m.out % 32 || m.in % 32)
        return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_lora_begin: model.layers.%d.%s is %d x %d (adapted matrices need dimensions that are multiples of 32)", l,
                       LORA_TARGET_NAMES[k], m.out, m.in);
      m.n_off = nrows; nrows += m.out;
      m.strip0 = strips;
      strips += (m.out + fv::LORA_STRIP_ROWS - 1) / fv::LORA_STRIP_ROWS;
      lc.kind = lg[k].kind; lc.mat[lg[k].part] = (int)mats.size();
      mats.push_back(m);
      adapted = true;
      fv::LoraDirectPack& pk = packs[(size_t)l * 4 + lg[k].which];
      if (pk.nm == 0) {
        pk.kind = lg[k].kind; pk.r = rank; pk.qd = qd; pk.kd = kd; pk.K = t.cols; pk.Np = t.rows;
        pk.slot_of_part[0] = pk.slot_of_part[1] = pk.slot_of_part[2] = -1;
      }
      pk.slot_of_part[lg[k].part] = pk.nm;
      pk.a_off[pk.nm] = m.a_off; pk.b_off[pk.nm] = m.b_off;
      ++pk.nm;
      pk.NCp = (pk.nm * rank + 31) / 32 * 32;
    }
    if (adapted) {
      lc.qd = qd; lc.kd = kd;
      lc.c.tile0 = ctiles; ctiles += ntile;
      lc.band0 = bands; bands += (t.rows + 63) / 64;
      cds.push_back(lc);
    } else {
      lc.c.tile0 = rtiles; rtiles += ntile;
      rest.push_back(lc.c);
    }
  }
  if (mats.empty()) return fv_fail(FV_ERR_ARG, "fv_train_lora_begin: no target matrix selected");
  // projection groups: consecutive matrices whose per-strip dA partial sums (strips x rank x in floats) fit the scratch together
  const size_t cap = (size_t)32 << 20;   // floats (128 MB); one matrix alone may exceed it
  ls.groups.clear();
  size_t scratch = 0;
  LoraGroup g{};
  size_t used = 0;
  for (size_t i = 0; i < mats.size(); ++i) {
    const int ns = (mats[i].out + fv::LORA_STRIP_ROWS - 1) / fv::LORA_STRIP_ROWS;
    const size_t need = (size_t)ns * rank * mats[i].in;
    if (g.m1 > g.m0 && used + need > cap) { ls.groups.push_back(g); g = LoraGroup{}; g.m0 = g.m1 = (int)i; g.strip_begin = mats[i].strip0; used = 0; }
    if (g.m1 == g.m0) { g.m0 = (int)i; g.strip_begin = mats[i].strip0; }
    mats[i].part_off = (long long)used;
    used += need; g.m1 = (int)i + 1; g.nstrips += ns; g.max_in = std::max(g.max_in, mats[i].in);
    scratch = std::max(scratch, used);
  }
  ls.groups.push_back(g);
  FV_TRY(upload(h, mats, &ls.mats)); ls.nmats = (int)mats.size();
  FV_TRY(upload(h, cds, &ls.cdesc)); ls.cn = (int)cds.size(); ls.ctiles = ctiles;
  FV_TRY(upload(h, rest, &ls.rest)); ls.rest_n = (int)rest.size(); ls.rest_tiles = rtiles;
  void* p = nullptr;
  if (scratch > ls.scratch_floats) {
    FV_TRY(dev_alloc(h, scratch * 4, &p));
    ls.scratch = static_cast<float*>(p); ls.scratch_floats = scratch;
  }
  ls.nbands = bands;
  if (dora && (size_t)nrows > ls.norm_floats) {
    FV_TRY(dev_alloc(h, (size_t)nrows * 4, &p));
    ls.norms = static_cast<float*>(p); ls.norm_floats = (size_t)nrows;
  }
  ls.front = lay.front; ls.total = lay.total;
  ls.packs = packs;
  return FV_OK;
}

// the direct backward's scratch: allocated once, for the largest step the handle admits (max_batch x (image tokens + max_text_tokens) rows)
int lora_direct_scratch(fv_handle* h, float** scratch, size_t* floats) {
  LoraState& ls = h->train.lora;
  const fv_model_desc& d = h->d;
  const int side = d.image_size >> (d.tower_stages + 1);
  const long rmax = (long)d.max_batch * (side * side + d.max_text_tokens);
  const int qkvw = (d.llm_heads + 2 * d.llm_kv_heads) * d.llm_head_dim;
  const int wmax = std::max(std::max(2 * d.llm_inter, qkvw), std::max(d.llm_hidden, d.llm_heads * d.llm_head_dim));
  const size_t need = fv::lora_direct_scratch_floats(rmax, ls.rank, wmax);
  if (need > ls.dscratch_floats) {
    void* p = nullptr;
    FV_HIP_CHECK(hipSetDevice(h->device));
    FV_TRY(dev_alloc(h, need * 4, &p));
    ls.dscratch = static_cast<float*>(p); ls.dscratch_floats = need;
  }
  *scratch = ls.dscratch; *floats = ls.dscratch_floats;
  return FV_OK;
}

// dA, dB of the adapters inside packed tensor `which` (0 q|k|v, 1 o, 2 gate/up, 3 down) of layer l; nothing at all when none of its matrices is a target
// from the gradient's fp16 rows dY16 [R][Np] and the kept activation X (split bf16 or fp16 rows)
int lora_direct_call(const DecCtx& c, int l, int which, const bf16_t* dY16, const ActOp& X, int R) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const LoraState& ls = h->train.lora;
  const fv::LoraDirectPack& pk = ls.packs[(size_t)l * 4 + which];
  if (pk.nm == 0) return FV_OK;
  // flop: the four skinny products; bytes: dY and X twice each
  FV_P(FV_FAM_GEMM, 4.0 * R * pk.NCp * ((double)pk.Np + pk.K), 2.0 * R * (2.0 * pk.Np + (X.kind == ActOp::SPLIT ? 4.0 : 2.0) * pk.K),
       fv::launch_lora_direct(pk, dY16, X.p, X.kind, X.ld, X.kind == ActOp::SPLIT ? pk.K : 0, R, c.lora_params, c.lora_grads, ls.scale, ls.dscratch, ls.dscratch_floats, s));
  return FV_OK;
}

int lora_check(fv_handle* h) {
  FV_TRY(train_check(h));
  if (!h->train.lora.on) return fv_fail(FV_ERR_STATE, "LoRA training not initialised: call fv_train_lora_begin first");
  return FV_OK;
}

bool lora_dora(const fv_handle* h) { return (h->train.lora.flags & FV_LORA_DORA) != 0; }

// the caller's device buffers of one entry point: none null (`what`: the word its message has always used), all 16-byte aligned
int check_buffers(const char* who, const char* what, std::initializer_list<const void*> bufs) {
  uintptr_t bits = 0;
  for (const void* b : bufs) {
    if (!b) return fv_fail(FV_ERR_ARG, "%s: null %s", who, what);
    bits |= (uintptr_t)b;
  }
  if (bits & 15) return fv_fail(FV_ERR_ARG, "%s: buffers must be 16-byte aligned", who);
  return FV_OK;
}

// DoRA: the row norms of W0 + s . B . A for these parameters into the handle's buffer (mag non-null: the magnitudes of that trainable buffer too)
int lora_refresh_norms(fv_handle* h, const float* master, const float* lora_params, float* mag, hipStream_t s) {
  LoraState& ls = h->train.lora;
  FV_TRY(fv::launch_lora_norms(ls.cdesc, ls.cn, ls.nbands, ls.mats, master, lora_params, ls.rank, ls.scale, ls.norms, mag, s));
  return FV_OK;
}

}  // namespace

extern "C" {

int fv_train_lora_begin(fv_handle* h, int rank, float alpha, int target_mask) { return fv_train_lora_begin_ex(h, rank, alpha, target_mask, 0); }

int fv_train_lora_begin_ex(fv_handle* h, int rank, float alpha, int target_mask, int flags) {
  HandleScope _hs(h);
  FV_TRY(train_check(h));
  if (flags & ~(FV_LORA_DORA | FV_LORA_RSLORA)) return fv_fail(FV_ERR_ARG, "fv_train_lora_begin_ex: flags 0x%x (FV_LORA_DORA = 1, FV_LORA_RSLORA = 2)", flags);
  if (rank < 1 || rank > 64) return fv_fail(FV_ERR_ARG, "fv_train_lora_begin: rank %d (1 .. 64)", rank);
  if (!(alpha > 0.f) || !std::isfinite(alpha)) return fv_fail(FV_ERR_ARG, "fv_train_lora_begin: alpha must be positive and finite");
  if (target_mask <= 0 || target_mask >= 128) return fv_fail(FV_ERR_ARG, "fv_train_lora_begin: target_mask 0x%x (bits 0 .. 6: q, k, v, o, gate, up, down; at least one)", target_mask);
  if (h->train.tower) return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_lora_begin: the tower is being trained (fv_train_tower_begin): adapters go with a frozen tower");
  LoraState& ls = h->train.lora;
  if (ls.on) {
    if (ls.rank == rank && ls.alpha == alpha && ls.mask == target_mask && ls.flags == flags) return FV_OK;
    if (ls.flags == 0 && flags == 0)
      return fv_fail(FV_ERR_STATE, "fv_train_lora_begin: already begun with rank %d, alpha %g, targets 0x%x", ls.rank, (double)ls.alpha, ls.mask);
    return fv_fail(FV_ERR_STATE, "fv_train_lora_begin: already begun with rank %d, alpha %g, targets 0x%x, flags 0x%x", ls.rank, (double)ls.alpha, ls.mask, ls.flags);
  }
  FV_HIP_CHECK(hipSetDevice(h->device));
  ls.rank = rank; ls.alpha = alpha; ls.mask = target_mask; ls.flags = flags;
  ls.scale = (flags & FV_LORA_RSLORA) ? alpha / sqrtf((float)rank) : alpha / (float)rank;
  const int rc = build_lora_tables(h);
  if (rc != FV_OK) { ls.flags = 0; return rc; }
  ls.on = true;
  return FV_OK;
}

int fv_train_lora_layout(fv_handle* h, fv_train_tensor* out, int max_tensors, int* n_tensors, int64_t* total_numel) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (!h->train.lora.on) return fv_fail(FV_ERR_STATE, "LoRA training not initialised: call fv_train_lora_begin first");
  const LoraLayout lay = lora_tensors(h, h->train.lora.rank, h->train.lora.mask, lora_dora(h));
  if (n_tensors) *n_tensors = (int)lay.tensors.size();
  if (total_numel) *total_numel = lay.total;
  return write_layout("fv_train_lora_layout", lay.tensors, out, max_tensors);
}

int fv_train_lora_project(fv_handle* h, const float* flat_grads_full, const float* lora_params, float* lora_grads, fv_stream st) {
  HandleScope _hs(h);
  FV_TRY(lora_check(h));
  FV_TRY(check_buffers("fv_train_lora_project", "buffer", {flat_grads_full, lora_params, lora_grads}));
  hipStream_t s = static_cast<hipStream_t>(st);
  const LoraState& ls = h->train.lora;
  // head and projector train in full: their gradients move over as they are (same offsets in both buffers)
  const bool dora = lora_dora(h);
  if (dora && !ls.master) return fv_fail(FV_ERR_STATE, "fv_train_lora_project: DoRA reads the row norms and the master of the last fv_train_lora_commit: commit these parameters first");
  FV_HIP_CHECK(hipMemcpyAsync(lora_grads, flat_grads_full, (size_t)ls.front * 4, hipMemcpyDeviceToDevice, s));
  for (const LoraGroup& g : ls.groups)
    FV_TRY(fv::launch_lora_project(ls.mats, g.m0, g.m1, g.strip_begin, g.nstrips, g.max_in, flat_grads_full, lora_params, lora_grads, ls.scratch, ls.rank, ls.scale, s,
                                   dora ? ls.master : nullptr, dora ? ls.norms : nullptr));
  return FV_OK;
}

int fv_train_lora_forward_backward(fv_handle* h, const float* flat_params, const float* lora_params, const void* tower_out, const int32_t* ids, const int32_t* lens,
                                   const float* states, const float* targets, int B, int T, int training, float dropout_p, uint64_t seed, uint64_t offset, void* ws,
                                   size_t ws_bytes, float* actions, float* loss, float* lora_grads, fv_stream st) {
  HandleScope _hs(h);
  FV_TRY(lora_check(h));
  FV_TRY(check_buffers("fv_train_lora_forward_backward", "pointer", {lora_params, lora_grads}));
  // refused HERE, before anything is enqueued
  if (lora_dora(h))
    return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_lora_forward_backward: not with DoRA (the magnitude's gradient needs the pre-bias GEMM outputs, which o / down do not keep): "
                                       "use fv_train_forward_backward + fv_train_lora_project");
  if (!fp16_backward(h))
    return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_lora_forward_backward: the direct LoRA backward runs on the default one-pass fp16 backward (fv_train_set_options 2, 1, k)");
  if (h->train.fwd_f16) return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_lora_forward_backward: not together with the fp16 training forward (fv_train_set_forward_f16)");
  // (a trained tower cannot reach this point: fv_train_lora_begin refuses after fv_train_tower_begin and the other way round, so lora_check has answered already)
  float* scr = nullptr;
  size_t scr_floats = 0;
  FV_TRY(lora_direct_scratch(h, &scr, &scr_floats));
  return train_forward_backward_impl(h, flat_params, tower_out, ids, lens, states, targets, B, T, training, dropout_p, seed, offset, ws, ws_bytes, actions, loss, nullptr,
                                     nullptr, nullptr, st, lora_params, lora_grads);
}

int fv_train_lora_commit(fv_handle* h, float* flat_params_master, const float* lora_params, fv_stream st) {
  HandleScope _hs(h);
  FV_TRY(lora_check(h));
  FV_TRY(check_buffers("fv_train_lora_commit", "buffer", {flat_params_master, lora_params}));
  hipStream_t s = static_cast<hipStream_t>(st);
  LoraState& ls = h->train.lora;
  FV_TRY(prompt_invalidate(h, s, true));   // the adapted operand images change
  // the master's head | projector front mirrors the trainable buffer's (fv_train_forward_backward reads the head there); nothing else of it is written
  FV_HIP_CHECK(hipMemcpyAsync(flat_params_master, lora_params, (size_t)ls.front * 4, hipMemcpyDeviceToDevice, s));
  const int f16t = h->train.grad_split == 2 ? 1 : 0;
  FV_TRY(fv::launch_commit(ls.rest, ls.rest_n, ls.rest_tiles, flat_params_master, f16t, h->f16_flags, s));
  const bool dora = lora_dora(h);
  if (dora) {
    FV_TRY(lora_refresh_norms(h, flat_params_master, lora_params, nullptr, s));
    ls.master = flat_params_master;
  }
  FV_TRY(fv::launch_lora_commit(ls.cdesc, ls.cn, ls.ctiles, ls.mats, flat_params_master, lora_params, ls.rank, ls.scale, f16t, h->f16_flags, s, dora ? ls.norms : nullptr));
  return FV_OK;
}

int fv_train_lora_merge(fv_handle* h, float* flat_params_master, const float* lora_params, fv_stream st) {
  HandleScope _hs(h);
  FV_TRY(lora_check(h));
  FV_TRY(check_buffers("fv_train_lora_merge", "buffer", {flat_params_master, lora_params}));
  hipStream_t s = static_cast<hipStream_t>(st);
  LoraState& ls = h->train.lora;
  FV_TRY(prompt_invalidate(h, s, true));   // (the merged master reaches the operand images with its next commit; the slot goes now)
  FV_HIP_CHECK(hipMemcpyAsync(flat_params_master, lora_params, (size_t)ls.front * 4, hipMemcpyDeviceToDevice, s));
  const bool dora = lora_dora(h);
  if (dora) {     // the norms of the master BEFORE it is overwritten; they describe neither buffer afterwards: the next commit refreshes them
    FV_TRY(lora_refresh_norms(h, flat_params_master, lora_params, nullptr, s));
    ls.master = nullptr;
  }
  FV_TRY(fv::launch_lora_merge(ls.cdesc, ls.cn, ls.ctiles, ls.mats, flat_params_master, lora_params, ls.rank, ls.scale, s, dora ? ls.norms : nullptr));
  return FV_OK;
}

int fv_train_lora_init_magnitude(fv_handle* h, const float* flat_params_master, float* lora_params, fv_stream st) {
  HandleScope _hs(h);
  FV_TRY(lora_check(h));
  if (!lora_dora(h)) return fv_fail(FV_ERR_STATE, "fv_train_lora_init_magnitude: LoRA mode was begun without FV_LORA_DORA");
  FV_TRY(check_buffers("fv_train_lora_init_magnitude", "buffer", {flat_params_master, lora_params}));
  FV_TRY(prompt_invalidate(h, static_cast<hipStream_t>(st), true));
  h->train.lora.master = nullptr;     // (the norm buffer now describes these buffers, but no commit of them has run)
  return lora_refresh_norms(h, flat_params_master, lora_params, lora_params, static_cast<hipStream_t>(st));
}

}  // extern "C"
