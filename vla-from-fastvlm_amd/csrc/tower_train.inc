// tower_train.inc -- host side of the TOWER half of the unfrozen-backbone training slice (SURVEY.md section 8f-4), included by engine.hip
// after train_path.inc.
//
// What is trained: the FastViT-HD tower in its re-parameterised (inference) form -- exactly the tensors the forward kernels consume: the stem's
// three convolutions, every RepMixer's folded 3x3, every ConvFFN (7x7 with its BatchNorm folded in, fc1, fc2, layer scale), the attention blocks
// (LayerNormChannel, qkv, proj, both layer scales), RepCPE, PatchEmbed (7x7 stride 2 + 1x1), conv_exp + SE.  The reference never reaches this
// (model/fastvlm_adapter.py:501; its knob is fastvla/configuration_fastvla.py:23, applied at model/fastvlm_adapter.py:170-173); the step body is
// training/trainer.py:171-182 over all parameters.  Oracle: torch autograd over oracle/fastvit_hd.py (tests/test_gpu_train_tower.py).
//
// Parameters.  The tower's tensors are APPENDED to the flat fp32 master of train_path.inc (after the decoder's final norm), in forward order, in the
// library's own layouts (depthwise weights tap-major [k*k][C], packing 3; the stem's dense 3x3 as [27][C0], packing 4; matrices [N][K]); gradient
// buckets one per stem / stage / PatchEmbed / conv_exp, reported through the same fv_bucket_cb in backward order.  fv_train_commit refreshes, in ONE
// launch over a table of operations, every operand image the forward and backward kernels read: fp32 copies, bf16 matrices, the packed MFMA images
// (Toeplitz tables, the fused ConvFFN's weight stream, the stem's [C0][64] image) through gather tables derived ONCE from the host packers themselves
// (pack(ones) gives each destination element's coefficient, pack(index + 1) its source), and the transposed fp16 dgrad operands (fc2 / proj with their
// layer scale folded in).
//
// Forward = the inference kernels, through the SAME unit bodies as the inference walk (engine.hip: mixer_convs, ffn_pointwise, attn_mixer, ...), writing
// every unit's tensors into a caller-owned stash instead of ping-pong buffers.  Backward, per unit, in fp16 operands carrying the loss scale
// (train_path.inc).  The ConvFFN's hidden is not kept: where the forward ran the fused 32x32x16 kernel's STASH instance, its pre-activation / 4 travels
// in the stash ([M][4C] fp16) and ONE dgrad GEMM leaves both gelu(a) and d a = (dout ls W2) gelu'(a) (FV_EPI_MUL_GELUP); only a block without that stash
// (the attention blocks, widths the 32x32x16 kernel lacks) recomputes the hidden by a GEMM of its own (FV_EPI_GELU_GRAD).  Dgrads are NT GEMMs against
// the transposed fp16 copies (FV_EPI_MUL_AUX / FV_EPI_F16 epilogues write the next operand directly); weight gradients are TN GEMMs over the pixel
// rows, cut into up to 32 K ranges; layer-scale gradients fall out of the UN-scaled weight gradient (ls_grads_kernel) without another pass over the
// pixels; everything else in tower_bwd_kernels.hip.

namespace {

enum {   // tensor roles inside a unit (index into TowerUnitOffs::o)
  R_W0 = 0, R_B0, R_W1, R_B1, R_W2, R_B2,                                                   // stem
  R_CW = 0, R_CB,                                                                            // RepCPE
  R_MW = 0, R_MB, R_DW, R_DB, R_F1W, R_F1B, R_F2W, R_F2B, R_LS,                              // RepMixer block (R_DW .. R_LS shared with the attention block)
  R_LNW = 9, R_LNB, R_QKVW, R_PW, R_PB, R_LS1,                                               // attention block (+ R_DW .. R_LS)
  R_LKW = 0, R_LKB, R_PWW, R_PWB,                                                            // PatchEmbed
  R_EW = 0, R_EB, R_S1W, R_S1B, R_S2W, R_S2B,                                                // conv_exp + SE
  R_MAX = 16
};

struct TowerTensor {
  std::string name;
  int rows = 1, cols = 0, bucket = 0, packing = 0, unit = 0, role = 0;
  float* lib_f32 = nullptr;     // the library's fp32 copy (vectors, depthwise / stem / SE weights)
  bf16_t* lib_bf16 = nullptr;   // ... or its bf16 [rows][cols] copy (dense matrices)
  int64_t off = 0;
};
struct TowerUnitOffs { int64_t o[R_MAX]; };

struct TUnit { int kind, stage, j, H, C, Ho, Co; size_t out, a, b, c, d, e; };
struct TowerTrainPlan {
  int B = 0;
  std::vector<TUnit> u;   // tower_units order, then the head (conv_exp + SE)
  size_t se, ga, gb, gc, hh, gp, t16, dt, pre, p16, f32a, f32b, stats, scr, splitk, splitk_bytes, total;
};

int tower_bucket_base(const fv_handle* h) { return TB_LAYER0 + h->d.llm_layers + 1; }
int tower_bucket_count(const fv_handle* h) { return 2 * h->d.tower_stages + 1; }

// every trainable tower tensor in forward order (offsets not yet assigned)
std::vector<TowerTensor> tower_tensor_list(fv_handle* h) {
  const fv_model_desc& d = h->d;
  Tower& tw = h->tw;
  std::vector<TowerTensor> out;
  const std::string vt = VT;
  const int base = tower_bucket_base(h);
  int unit = 0;
  auto add = [&](const std::string& n, int rows, int cols, int bucket, int packing, int role, float* f32, bf16_t* b16) {
    TowerTensor t;
    t.name = n; t.rows = rows; t.cols = cols; t.bucket = bucket; t.packing = packing; t.unit = unit; t.role = role; t.lib_f32 = f32; t.lib_bf16 = b16;
    out.push_back(t);
  };
  const int C0 = d.tower_dims[0];
  add(vt + "patch_embed.0.reparam_conv.weight", 27, C0, base, 4, R_W0, tw.stem0_w, nullptr);
  add(vt + "patch_embed.0.reparam_conv.bias", 1, C0, base, 0, R_B0, tw.stem0_b, nullptr);
  add(vt + "patch_embed.1.reparam_conv.weight", 9, C0, base, 3, R_W1, tw.stem1_w, nullptr);
  add(vt + "patch_embed.1.reparam_conv.bias", 1, C0, base, 0, R_B1, tw.stem1_b, nullptr);
  add(vt + "patch_embed.2.reparam_conv.weight", C0, C0, base, 0, R_W2, nullptr, tw.stem2_w);
  add(vt + "patch_embed.2.reparam_conv.bias", 1, C0, base, 0, R_B2, tw.stem2_b, nullptr);
  ++unit;
  auto add_ffn = [&](const std::string& pre, FFN& f, int C, int bucket, const std::string& ls_name) {
    const int hid = C * d.tower_mlp_ratio;
    add(pre + "convffn.conv.folded.weight", 49, C, bucket, 3, R_DW, f.dw_w, nullptr);   // conv.conv.weight with the BatchNorm folded in (load_ffn)
    add(pre + "convffn.conv.folded.bias", 1, C, bucket, 0, R_DB, f.dw_b, nullptr);
    add(pre + "convffn.fc1.weight", hid, C, bucket, 0, R_F1W, nullptr, f.fc1_w);
    add(pre + "convffn.fc1.bias", 1, hid, bucket, 0, R_F1B, f.fc1_b, nullptr);
    add(pre + "convffn.fc2.weight", C, hid, bucket, 0, R_F2W, nullptr, f.fc2_w);
    add(pre + "convffn.fc2.bias", 1, C, bucket, 0, R_F2B, f.fc2_b, nullptr);
    add(pre + ls_name, 1, C, bucket, 0, R_LS, f.ls, nullptr);
  };
  int idx = 0;
  for (int i = 0; i < d.tower_stages; ++i) {
    const int C = d.tower_dims[i], bs = base + 1 + 2 * i;
    if (d.tower_is_attn[i]) {
      const std::string pre = vt + "network." + std::to_string(idx++) + ".";
      add(pre + "reparam_conv.weight", 49, C, bs, 3, R_CW, tw.cpes[i].w, nullptr);
      add(pre + "reparam_conv.bias", 1, C, bs, 0, R_CB, tw.cpes[i].b, nullptr);
      ++unit;
    }
    const int sidx = idx++;
    for (int j = 0; j < d.tower_layers[i]; ++j) {
      const std::string pre = vt + "network." + std::to_string(sidx) + "." + std::to_string(j) + ".";
      Block& b = tw.stages[i][j];
      if (d.tower_is_attn[i]) {
        add_ffn(pre, b.ffn, C, bs, "layer_scale_2");
        add(pre + "norm.weight", 1, C, bs, 0, R_LNW, b.ln_w, nullptr);
        add(pre + "norm.bias", 1, C, bs, 0, R_LNB, b.ln_b, nullptr);
        add(pre + "token_mixer.qkv.weight", 3 * C, C, bs, 0, R_QKVW, nullptr, b.qkv_w);
        add(pre + "token_mixer.proj.weight", C, C, bs, 0, R_PW, nullptr, b.proj_w);
        add(pre + "token_mixer.proj.bias", 1, C, bs, 0, R_PB, b.proj_b, nullptr);
        add(pre + "layer_scale_1", 1, C, bs, 0, R_LS1, b.ls1, nullptr);
      } else {
        add(pre + "token_mixer.reparam_conv.weight", 9, C, bs, 3, R_MW, b.mix_w, nullptr);
        add(pre + "token_mixer.reparam_conv.bias", 1, C, bs, 0, R_MB, b.mix_b, nullptr);
        add_ffn(pre, b.ffn, C, bs, "layer_scale");
      }
      ++unit;
    }
    if (i + 1 < d.tower_stages) {
      const int C2 = d.tower_dims[i + 1], bd = base + 2 + 2 * i;
      const std::string pre = vt + "network." + std::to_string(idx++) + ".proj.";
      add(pre + "0.lkb_reparam.weight", 49, C2, bd, 3, R_LKW, tw.downs[i].lk_w, nullptr);
      add(pre + "0.lkb_reparam.bias", 1, C2, bd, 0, R_LKB, tw.downs[i].lk_b, nullptr);
      add(pre + "1.reparam_conv.weight", C2, C2, bd, 0, R_PWW, nullptr, tw.downs[i].pw_w);
      add(pre + "1.reparam_conv.bias", 1, C2, bd, 0, R_PWB, tw.downs[i].pw_b, nullptr);
      ++unit;
    }
  }
  const int CO = d.tower_out_dim, RD = d.tower_se_rd, bh = base + 2 * d.tower_stages;
  add(vt + "conv_exp.reparam_conv.weight", 9, CO, bh, 3, R_EW, tw.exp_w, nullptr);
  add(vt + "conv_exp.reparam_conv.bias", 1, CO, bh, 0, R_EB, tw.exp_b, nullptr);
  add(vt + "conv_exp.se.reduce.weight", RD, CO, bh, 0, R_S1W, tw.se_w1, nullptr);
  add(vt + "conv_exp.se.reduce.bias", 1, RD, bh, 0, R_S1B, tw.se_b1, nullptr);
  add(vt + "conv_exp.se.expand.weight", CO, RD, bh, 0, R_S2W, tw.se_w2, nullptr);
  add(vt + "conv_exp.se.expand.bias", 1, CO, bh, 0, R_S2B, tw.se_b2, nullptr);
  return out;
}

// called by train_tensors (train_path.inc) when the tower is trainable: appends the tower's tensors behind the decoder's
void append_tower_tensors(fv_handle* h, std::vector<TrainTensor>& out, int64_t& off) {
  for (const TowerTensor& tt : tower_tensor_list(h)) {
    TrainTensor t;
    t.name = tt.name; t.off = off; t.rows = tt.rows; t.cols = tt.cols; t.numel = (int64_t)tt.rows * tt.cols; t.bucket = tt.bucket; t.packing = tt.packing;
    t.lib = nullptr;   // (refreshed by the tower's own commit table, not by CommitDesc)
    t.is_mat = tt.lib_bf16 != nullptr;
    off += (t.numel + 3) / 4 * 4;
    out.push_back(t);
  }
}

// (unit, role) -> offset in the flat master / gradient; and the tensors with their offsets
std::vector<TowerTensor> tower_tensors_with_offsets(fv_handle* h, std::vector<TowerUnitOffs>* offs) {
  int64_t total = 0;
  const std::vector<TrainTensor> all = train_tensors(h, &total);
  std::vector<TowerTensor> tl = tower_tensor_list(h);
  const size_t first = all.size() - tl.size();
  int nu = 0;
  for (size_t i = 0; i < tl.size(); ++i) { tl[i].off = all[first + i].off; nu = std::max(nu, tl[i].unit + 1); }
  if (offs) {
    offs->assign(nu, TowerUnitOffs{});
    for (TowerUnitOffs& u : *offs) for (int r = 0; r < R_MAX; ++r) u.o[r] = -1;
    for (const TowerTensor& t : tl) (*offs)[t.unit].o[t.role] = t.off;
  }
  return tl;
}

// ---- gather tables: the host packers run on coefficient / index probes --------------------------------------------------------------------
int make_gtab(fv_handle* h, const std::string& key, size_t n_src, size_t n_dst, const std::function<void(const float*, float*)>& pack, GTab* out) {
  auto it = h->train.gtabs.find(key);
  if (it != h->train.gtabs.end()) { *out = it->second; return FV_OK; }
  if (n_src >= ((size_t)1 << 22)) return fv_fail(FV_ERR_UNSUPPORTED, "gather table %s: %zu source elements (limit 2^22)", key.c_str(), n_src);
  std::vector<float> ones(n_src, 1.0f), ramp(n_src), c(n_dst, 0.f), v(n_dst, 0.f);
  for (size_t i = 0; i < n_src; ++i) ramp[i] = (float)(i + 1);
  pack(ones.data(), c.data());
  pack(ramp.data(), v.data());
  std::vector<int> idx(n_dst);
  for (size_t i = 0; i < n_dst; ++i) {
    if (c[i] == 0.f) { idx[i] = -1; continue; }
    const float q = v[i] / c[i];
    const long j = std::lround(q) - 1;
    if (j < 0 || (size_t)j >= n_src || std::fabs(q - (float)(j + 1)) > 1e-3f)
      return fv_fail(FV_ERR_UNSUPPORTED, "gather table %s: destination %zu is not one scaled source element (%g / %g)", key.c_str(), i, (double)v[i], (double)c[i]);
    idx[i] = (int)j;
  }
  GTab g;
  g.n = n_dst;
  void* p = nullptr;
  FV_TRY(dev_alloc(h, n_dst * 4, &p)); g.idx = static_cast<int*>(p);
  FV_TRY(dev_alloc(h, n_dst * 4, &p)); g.coef = static_cast<float*>(p);
  FV_HIP_CHECK(hipMemcpy(g.idx, idx.data(), n_dst * 4, hipMemcpyHostToDevice));
  FV_HIP_CHECK(hipMemcpy(g.coef, c.data(), n_dst * 4, hipMemcpyHostToDevice));
  h->train.gtabs[key] = g;
  *out = g;
  return FV_OK;
}

// ---- workspace plan ------------------------------------------------------------------------------------------------------------------------
TowerTrainPlan plan_tower_train(const fv_handle* h, int B) {
  const fv_model_desc& d = h->d;
  TowerTrainPlan p{};
  p.B = B;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += align_up(bytes + 256); return r; };
  const size_t S = d.image_size;
  const int C0 = d.tower_dims[0], CO = d.tower_out_dim;
  size_t max_io = 0, max_hid = 0, max_rowsw = 0, max_t16 = 0;   // largest unit input / output (elements), largest [rows][4C] (elements), widest row, largest [rows][C + 8]
  for (const UnitInfo& q : tower_units(d, true)) {
    TUnit u{q.kind, q.stage, q.j, q.in_side, q.in_channels, q.side, q.channels, 0, 0, 0, 0, 0, 0};
    const int C = u.C;
    const size_t M = (size_t)B * u.H * u.H, out = (size_t)B * u.Ho * u.Ho * u.Co * 2;   // input rows (the stem: pixels), output bytes
    if (u.kind != TK_STEM) {
      max_io = std::max(max_io, M * C);
      max_t16 = std::max(max_t16, M * (C + 8));
      max_rowsw = std::max(max_rowsw, (size_t)C * d.tower_mlp_ratio);
    }
    if (u.kind == TK_STEM) {
      const size_t half = (size_t)B * (S / 2) * (S / 2) * C0;   // the first conv's output h0
      u.a = take(half * 2);
      u.b = take(out);
      max_hid = std::max(max_hid, half);   // dL/dh0 borrows the hidden-sized scratch
    } else if (u.kind == TK_BLOCK) {
      if (d.tower_is_attn[u.stage]) {
        u.a = take(M * C * 2); u.b = take(M * 3 * C * 2); u.c = take(M * C * 2); u.d = take(M * C * 2); u.e = take(M * C * 2);
      } else {
        u.a = take(M * C * 2); u.b = take(M * C * 2);
        // the fused ConvFFN's pre-activation travels from the forward to the backward (a / 4 as fp16 [M][4C]: convffn32.hip STASH) -- 0.7 GB per image at
        // 1024^2 -- exactly where ffn_pointwise will run the STASH instance.  (c == 0: the backward recomputes it by a GEMM of its own.)
        if (ffn_stash_ok(h, h->tw.stages[u.stage][u.j].ffn, (int)M, C) && !fv_ab_env("FASTVLA_NO_FFN_STASH")) u.c = take(M * C * d.tower_mlp_ratio * 2);
      }
      max_hid = std::max(max_hid, M * C * d.tower_mlp_ratio);
    } else if (u.kind == TK_DOWN || u.kind == TK_HEAD) {
      u.a = take(out);   // PatchEmbed's h1; the head's conv_exp output
    }
    if (u.kind == TK_HEAD) max_rowsw = std::max(max_rowsw, (size_t)CO);
    else u.out = take(out);   // (the head writes the caller's tower_out)
    max_io = std::max(max_io, out / 2);
    p.u.push_back(u);
  }
  p.se = take((size_t)B * (2 * CO + d.tower_se_rd) * 4);
  // scratch: row buffers carry 64 rows of the widest row as slack (the TN weight gradients contract over rows padded to 64 with zeros)
  const size_t slack = 64 * max_rowsw * 2;
  p.ga = take(max_io * 2 + slack); p.gb = take(max_io * 2 + slack); p.gc = take(max_io * 2 + slack);
  p.hh = take(max_hid * 2 + slack); p.gp = take(max_hid * 2 + slack);
  p.t16 = take(std::max(max_io, max_t16) * 2 + slack);   // (fc1's operand rows carry 8 more columns)
  p.dt = take(max_io * 2 + slack); p.pre = take(max_io * 2 + slack);
  p.p16 = take((size_t)B * (S / 2) * (S / 2) * 32 * 2 + 64 * 32 * 2);   // the stem's fp16 patch rows
  size_t wmax = 0, cmax = 0;   // largest weight-gradient matrix, widest channel count
  for (int i = 0; i < d.tower_stages; ++i) {
    const size_t C = d.tower_dims[i];
    wmax = std::max(wmax, C * C * d.tower_mlp_ratio);
    cmax = std::max(cmax, C * d.tower_mlp_ratio);
  }
  cmax = std::max(cmax, (size_t)CO);
  p.f32a = take((wmax + 8 * cmax) * 4);
  p.f32b = take(cmax * 4);
  // per-image attention statistics
  size_t stats = 0, scr = (size_t)fv::TOWER_COLSUM_CHUNKS * cmax;
  int H = (int)S / 4;
  scr = std::max(scr, fv::stem0_wgrad_scratch_floats(B, (int)S, C0));
  scr = std::max(scr, fv::dw_bwd_scratch_floats(B, (int)S / 4, (int)S / 4, C0, 3));
  for (int i = 0; i < d.tower_stages; ++i) {
    const int C = d.tower_dims[i];
    scr = std::max(scr, fv::dw_bwd_scratch_floats(B, H, H, C, 7));
    if (d.tower_is_attn[i]) {
      stats = std::max(stats, (size_t)2 * B * (C / d.tower_head_dim) * H * H);
      scr = std::max(scr, fv::ln_bwd_scratch_floats((long)B * H * H, C));
    }
    if (i + 1 < d.tower_stages) { scr = std::max(scr, fv::dw_bwd_scratch_floats(B, H / 2, H / 2, d.tower_dims[i + 1], 7)); H /= 2; }
  }
  scr = std::max(scr, fv::dw_bwd_scratch_floats(B, H, H, CO, 3));
  scr = std::max(scr, (size_t)B * (2 * CO + 2 * d.tower_se_rd));
  p.stats = take(stats * 4);
  p.scr = take(scr * 4);
  // split-K partial sums of the TN weight gradients: up to 128 ranges of the largest [C][4C] padded to 256-tiles
  size_t sk = 0;
  for (int i = 0; i < d.tower_stages; ++i) {
    const size_t C = d.tower_dims[i], N4 = (C * d.tower_mlp_ratio + 255) / 256 * 256;
    sk = std::max(sk, (size_t)128 * C * N4 * 4);
    sk = std::max(sk, (size_t)128 * C * d.tower_mlp_ratio * ((C + 255) / 256 * 256) * 4);
  }
  p.splitk_bytes = std::min(sk, (size_t)1 << 30);
  p.splitk = take(p.splitk_bytes);
  p.total = o;
  return p;
}

struct TowerCtx {   // everything one forward / backward call needs
  fv_handle* h; const TowerTrainPlan* tp; char* ws; hipStream_t s; float* grads; const std::vector<TowerUnitOffs>* offs; int B;
  template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
  float* G(int unit, int role) const { return grads + (*offs)[unit].o[role]; }
};

// tower part of the flat master <- the library's current copies (fp32 as they are, bf16 matrices widened exactly)
int tower_export(fv_handle* h, float* flat, hipStream_t s) {
  for (const TowerTensor& t : tower_tensors_with_offsets(h, nullptr)) {
    const size_t n = (size_t)t.rows * t.cols;
    if (t.lib_bf16) FV_TRY(fv::launch_bf16_to_f32(t.lib_bf16, flat + t.off, n, s));
    else FV_HIP_CHECK(hipMemcpyAsync(flat + t.off, t.lib_f32, n * 4, hipMemcpyDeviceToDevice, s));
  }
  return FV_OK;
}

int tower_check(fv_handle* h) {
  FV_TRY(train_check(h));
  if (!h->train.tower) return fv_fail(FV_ERR_STATE, "tower training not initialised: call fv_train_tower_begin first");
  return FV_OK;
}

// ---- forward of one unit into its stash: the unit bodies of engine.hip over the plan's buffers -----------------------------------------------------
int unit_forward(const TowerCtx& c, int ui, const bf16_t* in, bf16_t* out_override) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const Tower& tw = h->tw;
  const TUnit& u = c.tp->u[ui];
  const int B = c.B, H = u.H, C = u.C;
  bf16_t* out = out_override ? out_override : c.at<bf16_t>(u.out);
  bf16_t *a = c.at<bf16_t>(u.a), *b = c.at<bf16_t>(u.b);
  if (u.kind == TK_STEM) {
    FV_TRY(stem_convs(h, in, a, b, B, s));
    return stem_pw(h, b, out, B, s);
  }
  if (u.kind == TK_CPE) return dw_s1(h, in, tw.cpes[u.stage].w, tw.cpes[u.stage].t, tw.cpes[u.stage].b, out, B, H, C, 7, s);
  if (u.kind == TK_BLOCK) {
    const Block& blk = tw.stages[u.stage][u.j];
    bf16_t* hb = c.at<bf16_t>(c.tp->hh);
    const int M = B * H * H, hid = C * h->d.tower_mlp_ratio;
    if (!h->d.tower_is_attn[u.stage]) {   // a = x', b = t, c = the ConvFFN's stash where the plan reserved one
      FV_TRY(mixer_convs(h, blk, in, a, b, B, H, C, s));
      return ffn_pointwise(h, blk.ffn, b, a, out, hb, nullptr, 0, u.c ? c.at<bf16_t>(u.c) : nullptr, M, C, hid, s);
    }
    bf16_t *x1 = c.at<bf16_t>(u.d), *t = c.at<bf16_t>(u.e);   // a = y, b = qkv, c = o
    FV_TRY(attn_mixer(h, blk, in, a, b, c.at<bf16_t>(u.c), x1, B, H, C, s));
    FV_TRY(dw_s1(h, x1, blk.ffn.dw_w, blk.ffn.dw_t, blk.ffn.dw_b, t, B, H, C, 7, s));
    return ffn_pointwise(h, blk.ffn, t, x1, out, hb, nullptr, 0, nullptr, M, C, hid, s);
  }
  if (u.kind == TK_DOWN) return patch_embed(h, tw.downs[u.stage], in, a, out, B, H, C, u.Co, s);
  return tower_head(h, in, a, out, c.at<float>(c.tp->se), B, H, s);   // out_override is mandatory here: the caller's tower_out
}

// ---- backward helpers ----------------------------------------------------------------------------------------------------------------------
// out[Md][Nd] (fp32) = sum over `rows` of A[r][m] W[r][n]: fp16 row operands (row counts padded to 64 with zeros HERE: both buffers carry the slack)
int tower_wgrad(const TowerCtx& c, bf16_t* A, int lda, int Md, bf16_t* W, int ldw, int Nd, long rows, float* out, int ldo) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const long rp = (rows + 63) / 64 * 64;
  if (rp != rows) {
    FV_HIP_CHECK(hipMemsetAsync(A + rows * lda, 0, (size_t)(rp - rows) * lda * 2, s));
    FV_HIP_CHECK(hipMemsetAsync(W + rows * ldw, 0, (size_t)(rp - rows) * ldw * 2, s));
  }
  const long lim = (((long)1 << 31) - 1) / (2L * std::max(lda, ldw)) / 64 * 64;   // rows per launch (operands under 2 GiB)
  for (long r0 = 0; r0 < rp; r0 += lim) {
    const long n = std::min(lim, rp - r0);
    fv::GemmArgs g{A + r0 * lda, lda, W + r0 * ldw, Md, Nd, (int)n, nullptr, nullptr, r0 ? out : nullptr, ldo, out, ldo, r0 ? FV_EPI_RES_F32 : FV_EPI_F32, 0};
    g.tn = 1; g.ldw = ldw; g.f16 = 1;
    g.splitk_ws = c.tp->splitk_bytes ? c.at<float>(c.tp->splitk) : nullptr;
    g.splitk_bytes = c.tp->splitk_bytes;
    FV_TRY(gemm_p(h, g, s));
  }
  return FV_OK;
}
// out f16 [rows][N] = A f16 [rows][K] . WT16[N][K]^T, optionally times aux (FV_EPI_MUL_AUX)
// aux_preact_h != null: aux is the stashed pre-activation / 4 -- the epilogue multiplies by gelu'(4 aux) and leaves gelu(4 aux) in aux_preact_h (FV_EPI_MUL_GELUP)
int tower_dgrad(const TowerCtx& c, const bf16_t* A, int K, const bf16_t* WT16, int N, long rows, bf16_t* out, const bf16_t* aux = nullptr, bf16_t* aux_preact_h = nullptr) {
  fv::GemmArgs g{A, K, WT16, (int)rows, N, K, nullptr, nullptr, aux, aux ? N : 0, out, N, aux ? (aux_preact_h ? FV_EPI_MUL_GELUP : FV_EPI_MUL_AUX) : FV_EPI_F16, 0};
  g.f16 = 1; g.sat = c.h->f16_flags;
  g.stash = aux_preact_h;
  return gemm_p(c.h, g, c.s);
}
int tower_colsum(const TowerCtx& c, const bf16_t* in, int ld, long rows, int C, float* out) {
  return fv::launch_colsum16(in, ld, rows, C, out, c.at<float>(c.tp->scr), c.s);
}
int tower_rows16(const TowerCtx& c, const bf16_t* in_bf16, long rows, int C, bf16_t* out) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  FV_P(FV_FAM_ELT, 0.0, (double)rows * C * 4, fv::launch_rows_to_f16(in_bf16, 1, C, 0, out, C, rows, C, h->f16_flags, s));
  return FV_OK;
}

// backward of out = res + ls (.) (fc2(gelu(fc1(t) + b1)) + b2) from G = dL/dout (fp16 [M][C]): weight / bias / layer-scale gradients into the flat
// gradient, dL/dt (fp16 [M][C]) into the DT scratch.  (dL/dres = G is the caller's business.)
int ffn_backward(const TowerCtx& c, int ui, const FFN& f, const TowerTrainUnit& tu, const bf16_t* t, bf16_t* G, long M, int C, int hid, const bf16_t* stash_y = nullptr) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  bf16_t* hh = c.at<bf16_t>(c.tp->hh);
  bf16_t* gp = c.at<bf16_t>(c.tp->gp);
  bf16_t* t16 = c.at<bf16_t>(c.tp->t16);
  bf16_t* dt = c.at<bf16_t>(c.tp->dt);
  float* f32a = c.at<float>(c.tp->f32a);
  float* f32b = c.at<float>(c.tp->f32b);
  if (!stash_y) {   // the hidden again: gelu(a) (fc2's weight-gradient operand) and gelu'(a)
    fv::GemmArgs g{t, C, f.fc1_w, (int)M, hid, C, f.fc1_b, nullptr, nullptr, 0, hh, hid, FV_EPI_GELU_GRAD, 0};
    g.stash = gp; g.sat = h->f16_flags;
    FV_TRY(gemm_p(h, g, s));
  } else {          // ... unless the forward's fused kernel left a / 4 behind: d a = (dout ls W2) gelu'(a) AND gelu(a) from one read of it, no recompute GEMM
    FV_TRY(tower_dgrad(c, G, C, tu.fc2sT16, hid, M, gp, stash_y, hh));
  }
  FV_TRY(tower_colsum(c, G, C, M, C, f32b));                                          // sum_m dout
  FV_TRY(tower_wgrad(c, G, C, C, hh, hid, hid, M, f32a, hid));                        // sum_m dout (x) gelu(a): the un-scaled fc2 gradient
  FV_TRY(fv::launch_ls_grads(f32a, f32b, f.fc2_w, f.fc2_b, f.ls, c.G(ui, R_F2W), c.G(ui, R_F2B), c.G(ui, R_LS), C, hid, s));
  if (!stash_y) FV_TRY(tower_dgrad(c, G, C, tu.fc2sT16, hid, M, gp, gp));             // d a = (dout ls W2) gelu'(a), in place over gelu'(a)
  // fc1's weight AND bias gradient from one contraction over the pixels: t's fp16 rows carry a ones column ([M][C + 8]), so d a^T . [t | 1] = [dW1 | db1]
  // (a column sum of d a on its own is one more pass over the [M][4C] tensor)
  {
    const int ldt = C + 8;
    FV_P(FV_FAM_ELT, 0.0, (double)M * C * 4, fv::launch_rows_to_f16(t, 1, C, 0, t16, ldt, M, C, h->f16_flags, s));
    FV_TRY(fv::launch_ones_col(t16, ldt, C, M, s));
    float* wb = c.at<float>(c.tp->f32a);   // [hid][C + 8]
    FV_TRY(tower_wgrad(c, gp, hid, hid, t16, ldt, ldt, M, wb, ldt));
    FV_HIP_CHECK(hipMemcpy2DAsync(c.G(ui, R_F1W), (size_t)C * 4, wb, (size_t)ldt * 4, (size_t)C * 4, (size_t)hid, hipMemcpyDeviceToDevice, s));
    FV_HIP_CHECK(hipMemcpy2DAsync(c.G(ui, R_F1B), 4, wb + C, (size_t)ldt * 4, 4, (size_t)hid, hipMemcpyDeviceToDevice, s));
  }
  FV_TRY(tower_dgrad(c, gp, hid, tu.fc1T16, C, M, dt));                               // dL/dt
  return FV_OK;
}

int dw_backward(const TowerCtx& c, const bf16_t* x, const bf16_t* dy, const float* w, const bf16_t* res, bf16_t* dx, float* gw, float* gb, int Hi, int Ci, int k,
                int stride, int mult, const void* mfma_table = nullptr,   // mfma_table != null: the forward read bf16 taps (its Toeplitz table) -- so does the dgrad
                const bf16_t* flipped16 = nullptr) {                      // flipped16 != null: the input gradient on the marching MFMA kernel
  fv_handle* h = c.h; hipStream_t s = c.s;
  const int B = c.B;
  const int Ho = (Hi + 2 * (k / 2) - k) / stride + 1;
  if (dx) FV_P(FV_FAM_DWCONV, 2.0 * B * Ho * Ho * Ci * mult * k * k, 2.0 * B * Hi * Hi * Ci * (res ? 2 : 1) + 2.0 * B * Ho * Ho * Ci * mult,
               flipped16 ? fv::launch_dw_dgrad_mfma(dy, flipped16, res, dx, B, Hi, Hi, Ci, k, h->f16_flags, s)
                         : fv::launch_dw_dgrad(dy, w, res, dx, B, Hi, Hi, Ci, k, stride, mult, h->f16_flags, s, mfma_table ? 1 : 0));
  FV_P(FV_FAM_DWCONV, 2.0 * B * Ho * Ho * Ci * mult * k * k, 2.0 * B * Hi * Hi * Ci + 2.0 * B * Ho * Ho * Ci * mult,
       fv::launch_dw_wgrad(x, dy, gw, gb, c.at<float>(c.tp->scr), B, Hi, Hi, Ci, k, stride, mult, s));
  return FV_OK;
}

// backward of unit ui: gin = dL/d(its output) (fp16), gout = dL/d(its input) (fp16; null for the stem).  in = the unit's input as the forward saw it.
int unit_backward(const TowerCtx& c, int ui, const bf16_t* in, bf16_t* gin, bf16_t* gout) {
  fv_handle* h = c.h; hipStream_t s = c.s;
  const fv_model_desc& d = h->d;
  const Tower& tw = h->tw;
  const TUnit& u = c.tp->u[ui];
  const TowerTrainUnit& tu = h->train.tunits[ui];
  const int B = c.B;
  bf16_t* gc = c.at<bf16_t>(c.tp->gc);
  bf16_t* hh = c.at<bf16_t>(c.tp->hh);
  bf16_t* gp = c.at<bf16_t>(c.tp->gp);
  bf16_t* t16 = c.at<bf16_t>(c.tp->t16);
  bf16_t* dt = c.at<bf16_t>(c.tp->dt);
  bf16_t* pre = c.at<bf16_t>(c.tp->pre);
  float* f32a = c.at<float>(c.tp->f32a);
  float* f32b = c.at<float>(c.tp->f32b);
  if (u.kind == TK_HEAD) {
    const int H = u.H, CL = u.C, CO = u.Co, P = H * H, RD = d.tower_se_rd;
    const bf16_t* e = c.at<bf16_t>(u.a);
    FV_P(FV_FAM_ELT, 40.0 * B * P * CO, 8.0 * B * P * CO,
         fv::launch_se_bwd(e, gin, c.at<float>(c.tp->se), tw.se_w1, tw.se_w2, gp, c.G(ui, R_S1W), c.G(ui, R_S1B), c.G(ui, R_S2W), c.G(ui, R_S2B),
                           c.at<float>(c.tp->scr), B, P, CO, RD, h->f16_flags, s));
    return dw_backward(c, in, gp, tw.exp_w, nullptr, gout, c.G(ui, R_EW), c.G(ui, R_EB), H, CL, 3, 1, CO / CL);
  }
  if (u.kind == TK_CPE) {
    const Cpe& cp = tw.cpes[u.stage];
    return dw_backward(c, in, gin, cp.w, nullptr, gout, c.G(ui, R_CW), c.G(ui, R_CB), u.H, u.C, 7, 1, 1, cp.t, tu.mixF16);
  }
  if (u.kind == TK_BLOCK) {
    const Block& b = tw.stages[u.stage][u.j];
    const int H = u.H, C = u.C, hid = C * d.tower_mlp_ratio;
    const long M = (long)B * H * H;
    if (!d.tower_is_attn[u.stage]) {
      const bf16_t* xp = c.at<bf16_t>(u.a);
      const bf16_t* t = c.at<bf16_t>(u.b);
      FV_TRY(ffn_backward(c, ui, b.ffn, tu, t, gin, M, C, hid, u.c ? c.at<bf16_t>(u.c) : nullptr));
      // x' feeds the residual and the 7x7: dL/dx' = G + dw7^T(dL/dt); then the folded RepMixer 3x3
      FV_TRY(dw_backward(c, xp, dt, b.ffn.dw_w, gin, gc, c.G(ui, R_DW), c.G(ui, R_DB), H, C, 7, 1, 1, b.ffn.dw_t, tu.dwF16));
      return dw_backward(c, in, gc, b.mix_w, nullptr, gout, c.G(ui, R_MW), c.G(ui, R_MB), H, C, 3, 1, 1, b.mix_t, tu.mixF16);
    }
    const bf16_t* y = c.at<bf16_t>(u.a);
    const bf16_t* qkv = c.at<bf16_t>(u.b);
    const bf16_t* o = c.at<bf16_t>(u.c);
    const bf16_t* x1 = c.at<bf16_t>(u.d);
    const bf16_t* t = c.at<bf16_t>(u.e);
    FV_TRY(ffn_backward(c, ui, b.ffn, tu, t, gin, M, C, hid));
    FV_TRY(dw_backward(c, x1, dt, b.ffn.dw_w, gin, gc, c.G(ui, R_DW), c.G(ui, R_DB), H, C, 7, 1, 1, b.ffn.dw_t, tu.dwF16));      // gc = dL/dx1
    // x1 = x + ls1 (.) (proj(o) + pb)
    FV_TRY(tower_colsum(c, gc, C, M, C, f32b));
    FV_TRY(tower_rows16(c, o, M, C, t16));
    FV_TRY(tower_wgrad(c, gc, C, C, t16, C, C, M, f32a, C));
    FV_TRY(fv::launch_ls_grads(f32a, f32b, b.proj_w, b.proj_b, b.ls1, c.G(ui, R_PW), c.G(ui, R_PB), c.G(ui, R_LS1), C, C, s));
    FV_TRY(tower_dgrad(c, gc, C, tu.projsT16, C, M, dt));                                                     // dt = dL/do
    const int nh = C / d.tower_head_dim;
    FV_P(FV_FAM_ATTN, 10.0 * B * (double)(H * H) * (H * H) * C, 16.0 * M * C,
         fv::launch_tower_attn_bwd(qkv, 3 * C, dt, C, gp, 3 * C, c.at<float>(c.tp->stats), B, H * H, nh, 1.0f / std::sqrt((float)d.tower_head_dim), s));
    FV_TRY(tower_rows16(c, y, M, C, t16));
    FV_TRY(tower_wgrad(c, gp, 3 * C, 3 * C, t16, C, C, M, c.G(ui, R_QKVW), C));
    FV_TRY(tower_dgrad(c, gp, 3 * C, tu.qkvT16, C, M, hh));                                                   // hh = dL/dy
    FV_P(FV_FAM_NORM, 20.0 * M * C, 8.0 * M * C,
         fv::launch_ln_bwd(in, hh, b.ln_w, gc, gout, c.G(ui, R_LNW), c.G(ui, R_LNB), c.at<float>(c.tp->scr), M, C, d.ln_eps, h->f16_flags, s));
    return FV_OK;
  }
  // stem and PatchEmbed share their tail: ... -> dwconv s2 + GELU -> h1 -> 1x1 + GELU -> out
  const bool stem = u.kind == TK_STEM;
  const int S = d.image_size;
  const int Hi = stem ? S / 2 : u.H;                 // the depthwise conv's input side
  const int Ci = stem ? d.tower_dims[0] : u.C;
  const int C2 = u.Co, Ho = u.Ho;
  const int mult = C2 / Ci, k = stem ? 3 : 7;
  const long M2 = (long)B * Ho * Ho;
  const bf16_t* h1 = c.at<bf16_t>(stem ? u.b : u.a);
  const bf16_t* dwin = stem ? c.at<bf16_t>(u.a) : in;   // the depthwise conv's input (stem: the first conv's output h0)
  const bf16_t* pw_w = stem ? tw.stem2_w : tw.downs[u.stage].pw_w;
  const float* pw_b = stem ? tw.stem2_b : tw.downs[u.stage].pw_b;
  const float* lk_w = stem ? tw.stem1_w : tw.downs[u.stage].lk_w;
  const float* lk_b = stem ? tw.stem1_b : tw.downs[u.stage].lk_b;
  {
    fv::GemmArgs g{h1, C2, pw_w, (int)M2, C2, C2, pw_b, nullptr, nullptr, 0, nullptr, C2, FV_EPI_GELU_GRAD, 0};
    g.stash = gp; g.sat = h->f16_flags;
    FV_TRY(gemm_p(h, g, s));
  }
  FV_TRY(fv::launch_mul16(gin, gp, gp, (size_t)M2 * C2, h->f16_flags, s));                                    // gp = dL/d(1x1 pre-activation)
  FV_TRY(tower_rows16(c, h1, M2, C2, t16));
  FV_TRY(tower_wgrad(c, gp, C2, C2, t16, C2, C2, M2, c.G(ui, stem ? R_W2 : R_PWW), C2));
  FV_TRY(tower_colsum(c, gp, C2, M2, C2, c.G(ui, stem ? R_B2 : R_PWB)));
  FV_TRY(tower_dgrad(c, gp, C2, tu.pwT16, C2, M2, dt));                                                       // dt = dL/dh1
  // the depthwise conv's pre-activation again, by the kernel (and the tap precision) the forward used
  FV_P(FV_FAM_DWCONV, dw_flops(B, Ho, Ho, C2, k), 2.0 * B * Hi * Hi * Ci + 2.0 * M2 * C2,
       (!stem && tw.downs[u.stage].lk_t) ? fv::launch_dwconv_s2_mfma(dwin, tw.downs[u.stage].lk_t, lk_b, pre, B, Hi, Hi, Ci, 0, s)
                                         : fv::launch_dwconv(dwin, lk_w, lk_b, pre, B, Hi, Hi, Ci, k, 2, mult, 0, s));
  FV_TRY(fv::launch_gelu_grad_mul(dt, pre, dt, (size_t)M2 * C2, h->f16_flags, s));                            // dt = dL/d(depthwise pre-activation)
  if (!stem) return dw_backward(c, dwin, dt, lk_w, nullptr, gout, c.G(ui, R_LKW), c.G(ui, R_LKB), Hi, Ci, 7, 2, mult, tw.downs[u.stage].lk_t);
  FV_TRY(dw_backward(c, dwin, dt, lk_w, nullptr, hh, c.G(ui, R_W1), c.G(ui, R_B1), Hi, Ci, 3, 2, 1));          // hh = dL/dh0 (B, S/2, S/2, C0)
  const long M0 = (long)B * (S / 2) * (S / 2);
  if (tu.stem0_w32 && M0 % 64 == 0) {
    // the first conv's gradients on the GEMM kernels: patch rows P (fp16, ones column = the bias tap); a0 = P . [w | b]^T with gelu'(a0) left by the epilogue;
    // d a0 = dh0 gelu'(a0); [dW | db] = P^T . d a0 over the pixels (rows 0 .. 26 = the taps in the master's [27][C0] order, row 27 = the bias)
    bf16_t* p16 = c.at<bf16_t>(c.tp->p16);
    FV_P(FV_FAM_STEM, 0.0, (double)B * S * S * 8 + 64.0 * M0, fv::launch_stem_im2col16(in, p16, B, S, s));
    {
      fv::GemmArgs g{p16, 32, tu.stem0_w32, (int)M0, Ci, 32, tw.stem0_b, nullptr, nullptr, 0, nullptr, Ci, FV_EPI_GELU_GRAD, 0};
      g.f16 = 1; g.stash = gp; g.sat = h->f16_flags;
      FV_TRY(gemm_p(h, g, s));
    }
    FV_TRY(fv::launch_mul16(hh, gp, gp, (size_t)M0 * Ci, h->f16_flags, s));
    FV_TRY(tower_wgrad(c, p16, 32, 32, gp, Ci, Ci, M0, f32a, Ci));
    FV_HIP_CHECK(hipMemcpyAsync(c.G(ui, R_W0), f32a, (size_t)27 * Ci * 4, hipMemcpyDeviceToDevice, s));
    FV_HIP_CHECK(hipMemcpyAsync(c.G(ui, R_B0), f32a + (size_t)27 * Ci, (size_t)Ci * 4, hipMemcpyDeviceToDevice, s));
    return FV_OK;
  }
  FV_P(FV_FAM_STEM, 4.0 * B * (S / 2) * (S / 2) * 27 * Ci, (double)B * S * S * 8 + 2.0 * B * (S / 2) * (S / 2) * Ci,
       fv::launch_stem0_wgrad(in, tw.stem0_w, tw.stem0_b, hh, c.G(ui, R_W0), c.G(ui, R_B0), c.at<float>(c.tp->scr), B, S, Ci, s, tw.stem0_wp ? 1 : 0));
  return FV_OK;
}

// a tower bucket is complete: take the stream's own scale out of its gradients (they keep the loss scale, like every other tensor's), then report it
int tower_bucket_done(fv_handle* h, const std::vector<TowerTensor>& tl, int bucket, float* flat_grads, fv_bucket_cb cb, void* user, hipStream_t s) {
  int64_t lo = INT64_MAX, hi = 0;
  for (const TowerTensor& t : tl)
    if (t.bucket == bucket) { lo = std::min(lo, t.off); hi = std::max(hi, t.off + ((int64_t)t.rows * t.cols + 3) / 4 * 4); }
  if (hi <= lo) return FV_OK;
  FV_TRY(fv::launch_unscale_dev(flat_grads + lo, (size_t)(hi - lo), h->train.tscale, s));
  if (cb) cb(user, bucket, lo, hi - lo);
  return FV_OK;
}

}  // namespace

extern "C" {

int fv_train_tower_begin(fv_handle* h) {
  HandleScope _hs(h);
  FV_TRY(train_check(h));
  if (h->train.tower) return FV_OK;
  if (h->train.lora.on) return fv_fail(FV_ERR_UNSUPPORTED, "fv_train_tower_begin: LoRA mode is on (fv_train_lora_begin): adapters go with a frozen tower");
  const fv_model_desc& d = h->d;
  for (int i = 0; i < d.tower_stages; ++i)
    if (d.tower_dims[i] % 8 || (d.tower_is_attn[i] && d.tower_head_dim != 32))
      return fv_fail(FV_ERR_UNSUPPORTED, "tower training: stage widths must be multiples of 8 and the attention head_dim 32");
  FV_HIP_CHECK(hipSetDevice(h->device));
  h->train.tower = true;   // train_tensors now lists the tower
  // every early return below (an allocation, a gather table, the commit-table rebuild) leaves the handle as a decoder-only training handle: the flag, the unit
  // table and the device pointers the tower entry points dereference stay published only if the last statement is reached (ADVICE r5: a half-built handle
  // passed tower_check)
  struct Rollback {
    fv_handle* h; bool armed = true;
    ~Rollback() {
      if (!armed) return;
      h->train.tower = false;
      h->train.tunits.clear();
      h->train.tscale = nullptr; h->train.tower_ops = nullptr; h->train.tower_nops = 0; h->train.tower_blocks = 0;
      h->train.pj0T = nullptr; h->train.pj0T16 = nullptr;
      (void)build_commit_table(h);   // without the tower's rows again (device allocations stay on the handle's list and are freed with it)
    }
  } rollback{h};
  std::vector<TowerUnitOffs> offs;
  const std::vector<TowerTensor> tl = tower_tensors_with_offsets(h, &offs);
  Tower& tw = h->tw;
  const int nu = (int)offs.size();
  h->train.tunits.assign(nu, TowerTrainUnit{});
  std::vector<fv::TowerCommitOp> ops;
  int rc = FV_OK;
  auto op = [&](int kind, int64_t src, int64_t src2, void* dst, int64_t n, int rows, int cols, const GTab* g) {
    if (!dst) return;
    fv::TowerCommitOp o{};
    o.kind = kind; o.src_off = src; o.src2_off = src2; o.dst = dst; o.n = n; o.rows = rows; o.cols = cols;
    o.idx = g ? g->idx : nullptr; o.coef = g ? g->coef : nullptr;
    ops.push_back(o);
  };
  auto t16 = [&](size_t n) -> bf16_t* { void* p = nullptr; if (dev_alloc(h, n * 2, &p) != FV_OK) { rc = FV_ERR_HIP; return nullptr; } return static_cast<bf16_t*>(p); };
  auto toeplitz = [&](int C, int k, GTab* g) {
    return make_gtab(h, "toep" + std::to_string(k) + "_" + std::to_string(C), (size_t)k * k * C, fv::dwconv_toeplitz_elems(C, k),
                     [=](const float* a, float* b) { fv::dwconv_toeplitz_pack(a, b, C, k); }, g);
  };
  // the FLIPPED taps' Toeplitz table (the input gradient of a stride-1 depthwise conv is the conv with the mirrored kernel), as fp16, where the marching kernel serves the map
  auto toeplitz_flipped = [&](int C, int k, GTab* g) {
    return make_gtab(h, "toepF" + std::to_string(k) + "_" + std::to_string(C), (size_t)k * k * C, fv::dwconv_toeplitz_elems(C, k),
                     [=](const float* a, float* b) {
                       std::vector<float> f((size_t)k * k * C);
                       for (int t2 = 0; t2 < k * k; ++t2) memcpy(&f[(size_t)t2 * C], a + (size_t)(k * k - 1 - t2) * C, (size_t)C * 4);
                       fv::dwconv_toeplitz_pack(f.data(), b, C, k);
                     }, g);
  };
  auto flipped_table = [&](const TowerTensor& t, int C, int k, int side, bf16_t** dst) -> int {
    if (!fv::dw_dgrad_mfma_supported(side, side, C, k)) return FV_OK;
    GTab g;
    FV_TRY(toeplitz_flipped(C, k, &g));
    *dst = t16(g.n);
    op(5, t.off, 0, *dst, (int64_t)g.n, 0, 0, &g);
    return FV_OK;
  };
  const std::vector<UnitInfo> ui = tower_units(d, true);
  for (const TowerTensor& t : tl) {
    const int64_t n = (int64_t)t.rows * t.cols;
    TowerTrainUnit& tu = h->train.tunits[t.unit];
    if (t.lib_f32) op(0, t.off, 0, t.lib_f32, n, t.rows, t.cols, nullptr);
    if (t.lib_bf16) op(1, t.off, 0, t.lib_bf16, n, t.rows, t.cols, nullptr);
    const int kind = ui[t.unit].kind, stage = ui[t.unit].stage;
    const bool attn = kind == TK_BLOCK && d.tower_is_attn[stage];
    GTab g;
    if (kind == TK_STEM) {
      if (t.role == R_W0 && tw.stem0_wp) {
        const int C0 = t.cols;
        FV_TRY(make_gtab(h, "stem_" + std::to_string(C0), (size_t)27 * C0, (size_t)C0 * 64, [=](const float* a, float* b) { fv::stem_mfma_pack(a, b, C0); }, &g));
        op(2, t.off, 0, tw.stem0_wp, (int64_t)g.n, 0, 0, &g);
      }
      if (t.role == R_W2) { tu.pwT16 = t16((size_t)n); op(3, t.off, 0, tu.pwT16, n, t.rows, t.cols, nullptr); }
      if (t.role == R_W0) {   // [C0][32] fp16 image of the taps for the backward's recompute GEMM
        const int C0 = t.cols;
        const int64_t delta = offs[t.unit].o[R_B0] - t.off;
        FV_TRY(make_gtab(h, "stem32_" + std::to_string(C0) + "_" + std::to_string((long long)delta), (size_t)delta + C0, (size_t)C0 * 32,
                         [=](const float* a, float* o2) {
                           for (int co = 0; co < C0; ++co)
                             for (int k = 0; k < 32; ++k) o2[(size_t)co * 32 + k] = k < 27 ? a[(size_t)k * C0 + co] : 0.f;   // (column 27, the ones column of the patch rows, meets a zero: the bias enters the GEMM in fp32)
                         }, &g));
        tu.stem0_w32 = t16(g.n);
        op(tw.stem0_wp ? 5 : 6, t.off, 0, tu.stem0_w32, (int64_t)g.n, 0, 0, &g);
      }
    } else if (kind == TK_CPE) {
      if (t.role == R_CW && tw.cpes[stage].t) { FV_TRY(toeplitz(t.cols, 7, &g)); op(2, t.off, 0, tw.cpes[stage].t, (int64_t)g.n, 0, 0, &g); }
      if (t.role == R_CW) FV_TRY(flipped_table(t, t.cols, 7, ui[t.unit].side, &tu.mixF16));
    } else if (kind == TK_DOWN) {
      Down& dn = tw.downs[stage];
      if (t.role == R_LKW && dn.lk_t) {
        const int Cin = d.tower_dims[stage];
        FV_TRY(make_gtab(h, "s2toep_" + std::to_string(Cin), (size_t)49 * t.cols, fv::dwconv_s2_toeplitz_elems(Cin),
                         [=](const float* a, float* b) { fv::dwconv_s2_toeplitz_pack(a, b, Cin); }, &g));
        op(2, t.off, 0, dn.lk_t, (int64_t)g.n, 0, 0, &g);
      }
      if (t.role == R_PWW) { tu.pwT16 = t16((size_t)n); op(3, t.off, 0, tu.pwT16, n, t.rows, t.cols, nullptr); }
    } else if (kind == TK_BLOCK) {
      Block& b = tw.stages[stage][ui[t.unit].j];
      FFN& f = b.ffn;
      const int C = d.tower_dims[stage], hid = C * d.tower_mlp_ratio;
      if (!attn && t.role == R_MW && b.mix_t) { FV_TRY(toeplitz(C, 3, &g)); op(2, t.off, 0, b.mix_t, (int64_t)g.n, 0, 0, &g); }
      if (t.role == R_DW && f.dw_t) { FV_TRY(toeplitz(C, 7, &g)); op(2, t.off, 0, f.dw_t, (int64_t)g.n, 0, 0, &g); }
      if (!attn && t.role == R_MW) FV_TRY(flipped_table(t, C, 3, ui[t.unit].side, &tu.mixF16));
      if (t.role == R_DW) FV_TRY(flipped_table(t, C, 7, ui[t.unit].side, &tu.dwF16));
      if (t.role == R_F1W) {
        tu.fc1T16 = t16((size_t)n); op(3, t.off, 0, tu.fc1T16, n, t.rows, t.cols, nullptr);
        if (f.w2q) {   // the 32x32x16 fused kernel's stream reads fc1 AND fc2: one table over the span [fc1.weight .. fc2.weight]
          const int64_t delta = offs[t.unit].o[R_F2W] - t.off;
          const size_t span = (size_t)delta + (size_t)C * hid;
          FV_TRY(make_gtab(h, "ffn32_" + std::to_string(C) + "_" + std::to_string((long long)delta), span, (size_t)2 * hid * C,
                           [=](const float* a, float* o2) { fv::convffn32_pack(a, a + delta, o2, C); }, &g));
          op(2, t.off, 0, f.w2q, (int64_t)g.n, 0, 0, &g);
        }
      }
      if (t.role == R_F2W) {
        tu.fc2sT16 = t16((size_t)n); op(4, t.off, offs[t.unit].o[R_LS], tu.fc2sT16, n, t.rows, t.cols, nullptr);
        if (f.w2p) {
          FV_TRY(make_gtab(h, "w2p_" + std::to_string(C), (size_t)C * hid, (size_t)C * hid, [=](const float* a, float* o2) { fv::convffn_pack_w2(a, o2, C, hid); }, &g));
          op(2, t.off, 0, f.w2p, (int64_t)g.n, 0, 0, &g);
        }
      }
      if (attn && t.role == R_QKVW) { tu.qkvT16 = t16((size_t)n); op(3, t.off, 0, tu.qkvT16, n, t.rows, t.cols, nullptr); }
      if (attn && t.role == R_PW) { tu.projsT16 = t16((size_t)n); op(4, t.off, offs[t.unit].o[R_LS1], tu.projsT16, n, t.rows, t.cols, nullptr); }
    }
    if (rc != FV_OK) return rc;
  }
  {
    void* p = nullptr;
    FV_TRY(dev_alloc(h, 16, &p));
    h->train.tscale = static_cast<float*>(p);
    const float one[4] = {1.0f, 1.0f, 0.0f, 0.0f};
    FV_HIP_CHECK(hipMemcpy(h->train.tscale, one, 16, hipMemcpyHostToDevice));
  }
  int blk = 0;
  for (fv::TowerCommitOp& o : ops) { o.blk0 = blk; blk += (int)((o.n + 1023) / 1024); }
  void* dp = nullptr;
  FV_TRY(dev_alloc(h, ops.size() * sizeof(fv::TowerCommitOp), &dp));
  FV_HIP_CHECK(hipMemcpy(dp, ops.data(), ops.size() * sizeof(fv::TowerCommitOp), hipMemcpyHostToDevice));
  h->train.tower_ops = static_cast<fv::TowerCommitOp*>(dp); h->train.tower_nops = (int)ops.size(); h->train.tower_blocks = blk;
  // the projector's first Linear now has a consumer for its input gradient: its transposed copies (train_tensors lists them from here on)
  {
    const size_t n = (size_t)d.llm_hidden * d.tower_out_dim;
    void* p = nullptr;
    FV_TRY(dev_alloc(h, n * 2, &p)); h->train.pj0T = static_cast<bf16_t*>(p);
    FV_TRY(dev_alloc(h, n * 2, &p)); h->train.pj0T16 = static_cast<bf16_t*>(p);
    FV_TRY(fv::launch_transpose_to_bf16(tw.pj0_w, 1, d.tower_out_dim, h->train.pj0T, d.llm_hidden, 0, d.llm_hidden, d.llm_hidden, d.tower_out_dim, nullptr));
    FV_TRY(fv::launch_transpose_to_f16(tw.pj0_w, 1, d.tower_out_dim, 0, h->train.pj0T16, d.llm_hidden, d.llm_hidden, d.llm_hidden, d.tower_out_dim, h->f16_flags, nullptr));
    // fv_train_commit's descriptor table is rebuilt so that these follow the master too
    FV_TRY(build_commit_table(h));
  }
  FV_HIP_CHECK(hipDeviceSynchronize());
  // the transposed fp16 operands as of the weights loaded: run the tower's commit once from an exported master
  {
    int64_t total = 0;
    (void)train_tensors(h, &total);
    float* tmp = nullptr;
    FV_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&tmp), (size_t)total * 4));
    int erc = tower_export(h, tmp, nullptr);
    if (erc == FV_OK) erc = fv::launch_tower_commit(h->train.tower_ops, h->train.tower_nops, h->train.tower_blocks, tmp, h->f16_flags, nullptr);
    const hipError_t e = hipDeviceSynchronize();
    (void)hipFree(tmp);
    if (erc != FV_OK) return erc;
    FV_HIP_CHECK(e);
  }
  rollback.armed = false;
  return FV_OK;
}

int fv_train_tower_workspace_bytes(fv_handle* h, int B, size_t* out_bytes) {
  HandleScope _hs(h);
  if (!h || !out_bytes) return fv_fail(FV_ERR_ARG, "null argument");
  if (B <= 0 || B > h->d.max_batch) return fv_fail(FV_ERR_ARG, "fv_train_tower_workspace_bytes: bad B");
  *out_bytes = plan_tower_train(h, B).total;
  return FV_OK;
}

int fv_train_tower_forward(fv_handle* h, const void* pix, int B, void* tws, size_t tws_bytes, void* tower_out, fv_stream st) {
  HandleScope _hs(h);
  TrainScope _ts(h);
  FV_TRY(tower_check(h));
  if (!pix || !tws || !tower_out || B <= 0 || B > h->d.max_batch) return fv_fail(FV_ERR_ARG, "fv_train_tower_forward: bad argument");
  if ((uintptr_t)tws & 255) return fv_fail(FV_ERR_ARG, "fv_train_tower_forward: workspace must be 256-byte aligned");
  const TowerTrainPlan tp = plan_tower_train(h, B);
  if (tp.total > tws_bytes) return fv_fail(FV_ERR_STATE, "tower training workspace too small (%zu > %zu)", tp.total, tws_bytes);
  TowerCtx c{h, &tp, static_cast<char*>(tws), static_cast<hipStream_t>(st), nullptr, nullptr, B};
  const bf16_t* in = static_cast<const bf16_t*>(pix);
  const int nu = (int)tp.u.size();
  for (int ui = 0; ui < nu; ++ui) {
    const bool head = ui == nu - 1;
    FV_TRY(unit_forward(c, ui, in, head ? static_cast<bf16_t*>(tower_out) : nullptr));
    in = c.at<bf16_t>(tp.u[ui].out);
  }
  return FV_OK;
}

int fv_train_tower_backward(fv_handle* h, const void* pix, const void* d_tower_out, int B, void* tws, size_t tws_bytes, float* flat_grads, fv_bucket_cb cb,
                            void* user, fv_stream st) {
  HandleScope _hs(h);
  TrainScope _ts(h);
  FV_TRY(tower_check(h));
  if (!pix || !d_tower_out || !tws || !flat_grads || B <= 0 || B > h->d.max_batch) return fv_fail(FV_ERR_ARG, "fv_train_tower_backward: bad argument");
  if (((uintptr_t)tws & 255) || ((uintptr_t)flat_grads & 15) || ((uintptr_t)d_tower_out & 15)) return fv_fail(FV_ERR_ARG, "fv_train_tower_backward: misaligned buffer");
  const TowerTrainPlan tp = plan_tower_train(h, B);
  if (tp.total > tws_bytes) return fv_fail(FV_ERR_STATE, "tower training workspace too small (%zu > %zu)", tp.total, tws_bytes);
  std::vector<TowerUnitOffs> offs;
  const std::vector<TowerTensor> tl = tower_tensors_with_offsets(h, &offs);
  TowerCtx c{h, &tp, static_cast<char*>(tws), static_cast<hipStream_t>(st), flat_grads, &offs, B};
  const int nu = (int)tp.u.size();
  bf16_t* ga = c.at<bf16_t>(tp.ga);
  bf16_t* gb = c.at<bf16_t>(tp.gb);
  // the head reads the caller's gradient in place; from there the stream ping-pongs between ga and gb
  bf16_t* gin = const_cast<bf16_t*>(static_cast<const bf16_t*>(d_tower_out));
  bf16_t* gout = ga;
  const int base = tower_bucket_base(h);
  for (int ui = nu - 1; ui >= 0; --ui) {
    const bf16_t* in = ui == 0 ? static_cast<const bf16_t*>(pix) : c.at<bf16_t>(tp.u[ui - 1].out);
    FV_TRY(unit_backward(c, ui, in, gin, ui == 0 ? nullptr : gout));
    // bucket boundaries: the head; a stage's first unit (its RepCPE if it has one); a PatchEmbed; the stem
    const TUnit& u = tp.u[ui];
    bool done = false; int bucket = 0;
    if (u.kind == TK_HEAD) { done = true; bucket = base + 2 * h->d.tower_stages; }
    else if (u.kind == TK_STEM) { done = true; bucket = base; }
    else if (u.kind == TK_DOWN) { done = true; bucket = base + 2 + 2 * u.stage; }
    else if (u.kind == TK_CPE) { done = true; bucket = base + 1 + 2 * u.stage; }
    else if (u.kind == TK_BLOCK && u.j == 0 && !h->d.tower_is_attn[u.stage]) { done = true; bucket = base + 1 + 2 * u.stage; }
    if (done) FV_TRY(tower_bucket_done(h, tl, bucket, flat_grads, cb, user, c.s));
    gin = gout;
    gout = gout == ga ? gb : ga;
  }
  return FV_OK;
}

// ONE unit, teacher-forced (the parity tests): x_in = the unit's input (bf16 NHWC; the stem: letterboxed pixels (B,S,S,4)), g_out = dL/d(its output) in
// fp32 NHWC.  Runs the unit's forward into the stash, then its backward with g_out * gscale as the fp16 gradient.  y_out (bf16, optional) receives the unit's
// output; g_in (fp32 NHWC of the input, optional, null for the stem) = dL/d(input) (the gscale taken out again); the unit's weight gradients land in flat_grads
// at their fv_train_layout offsets, TIMES gscale.  unit = fv_vision_unit_info's index; the unit count itself = conv_exp + SE.
int fv_train_tower_unit(fv_handle* h, int unit, const void* x_in, const float* g_out, float gscale, int B, void* tws, size_t tws_bytes, void* y_out, float* g_in,
                        float* flat_grads, fv_stream st) {
  HandleScope _hs(h);
  TrainScope _ts(h);
  FV_TRY(tower_check(h));
  if (!x_in || !g_out || !tws || !flat_grads || B <= 0 || B > h->d.max_batch) return fv_fail(FV_ERR_ARG, "fv_train_tower_unit: bad argument");
  const TowerTrainPlan tp = plan_tower_train(h, B);
  if (tp.total > tws_bytes) return fv_fail(FV_ERR_STATE, "tower training workspace too small (%zu > %zu)", tp.total, tws_bytes);
  const int nu = (int)tp.u.size();
  if (unit < 0 || unit >= nu) return fv_fail(FV_ERR_ARG, "fv_train_tower_unit: unit %d out of range [0, %d]", unit, nu - 1);
  std::vector<TowerUnitOffs> offs;
  (void)tower_tensors_with_offsets(h, &offs);
  hipStream_t s = static_cast<hipStream_t>(st);
  TowerCtx c{h, &tp, static_cast<char*>(tws), s, flat_grads, &offs, B};
  const TUnit& u = tp.u[unit];
  const size_t n_out = (size_t)B * u.Ho * u.Ho * u.Co, n_in = (size_t)B * u.H * u.H * u.C;
  bf16_t* yo = u.kind == TK_HEAD ? c.at<bf16_t>(tp.pre) : c.at<bf16_t>(u.out);
  FV_TRY(unit_forward(c, unit, static_cast<const bf16_t*>(x_in), u.kind == TK_HEAD ? yo : nullptr));
  if (y_out) FV_HIP_CHECK(hipMemcpyAsync(y_out, yo, n_out * 2, hipMemcpyDeviceToDevice, s));
  bf16_t* ga = c.at<bf16_t>(tp.ga);
  bf16_t* gb = c.at<bf16_t>(tp.gb);
  FV_TRY(fv::launch_scale_to_f16(g_out, ga, n_out, gscale, h->f16_flags, s));
  FV_TRY(unit_backward(c, unit, static_cast<const bf16_t*>(x_in), ga, u.kind == TK_STEM ? nullptr : gb));
  if (g_in && u.kind != TK_STEM) FV_TRY(fv::launch_f16_to_f32(gb, g_in, n_in, 1.0f / gscale, s));
  return FV_OK;
}

// unit `unit`'s output (bf16 NHWC) as the last fv_train_tower_forward left it in tws (parity tests: teacher-forcing the oracle at every unit boundary)
int fv_train_tower_read_unit(fv_handle* h, int unit, int B, const void* tws, size_t tws_bytes, void* out, fv_stream st) {
  HandleScope _hs(h);
  FV_TRY(tower_check(h));
  if (!tws || !out || B <= 0 || B > h->d.max_batch) return fv_fail(FV_ERR_ARG, "fv_train_tower_read_unit: bad argument");
  const TowerTrainPlan tp = plan_tower_train(h, B);
  if (tp.total > tws_bytes) return fv_fail(FV_ERR_STATE, "tower training workspace too small (%zu > %zu)", tp.total, tws_bytes);
  if (unit < 0 || unit + 1 >= (int)tp.u.size()) return fv_fail(FV_ERR_ARG, "fv_train_tower_read_unit: unit %d out of range [0, %d)", unit, (int)tp.u.size() - 1);
  const TUnit& u = tp.u[unit];
  FV_HIP_CHECK(hipMemcpyAsync(out, static_cast<const char*>(tws) + u.out, (size_t)B * u.Ho * u.Ho * u.Co * 2, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(st)));
  return FV_OK;
}

int fv_train_set_tower_grad(fv_handle* h, void* d_tower_out_f16) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if ((uintptr_t)d_tower_out_f16 & 15) return fv_fail(FV_ERR_ARG, "fv_train_set_tower_grad: buffer must be 16-byte aligned");
  if (d_tower_out_f16 && !h->train.tower) return fv_fail(FV_ERR_STATE, "fv_train_set_tower_grad: call fv_train_tower_begin first");
  // A gradient handed to fv_train_tower_backward directly carries no extra scale; fv_train_forward_backward sets its own every step.  The reset happens only
  // when the binding CHANGES (re-binding the same buffer every step is a no-op): the blocking copy drains the null stream and is unordered against a
  // non-blocking caller stream's launch_unscale_dev of the previous step (ADVICE r5) -- a change of binding is a setup-time event, and the device is
  // synchronised around it so that no step in flight reads the scale while it is rewritten.
  if (h->train.d_tower_out == d_tower_out_f16) return FV_OK;
  h->train.d_tower_out = d_tower_out_f16;
  if (h->train.tscale) {
    const float one[2] = {1.0f, 1.0f};
    FV_HIP_CHECK(hipSetDevice(h->device));
    FV_HIP_CHECK(hipDeviceSynchronize());
    FV_HIP_CHECK(hipMemcpy(h->train.tscale, one, 8, hipMemcpyHostToDevice));
  }
  return FV_OK;
}

}  // extern "C"
