// head_path.inc -- the action expert's entry points (fv_head_*) and the temporal-ensembling ring's (fv_ensemble_*), included by engine.hip: argument checks,
// the handle's configuration (dataset statistics, loss, flow mode, guidance, draws) and the call into the launchers of head_kernels.hip, chunk_kernels.hip
// and flow_kernels.hip.
namespace {

// the head's parameter count, for the profiler's FLOP / byte estimates
double head_param_count(const fv_handle* h) { return (double)fv::head_offsets(h->hd).o[fv::HP_TOTAL]; }

// *scr <- the head's scratch inside the bound workspace for a call with B rows; `too_small`: the caller's message for a workspace bound for a smaller plan
int head_scratch(fv_handle* h, int B, const char* too_small, float** scr) {
  if (!h->ws) return fv_fail(FV_ERR_STATE, "workspace not bound: call fv_bind_workspace first");
  if (B > h->d.max_batch) return fv_fail(FV_ERR_ARG, "B=%d exceeds max_batch=%d", B, h->d.max_batch);
  const WsPlan wp = plan_ws(h, B, 1, 0);
  if (wp.total > h->ws_bytes) return fv_fail(FV_ERR_STATE, "%s", too_small);
  *scr = reinterpret_cast<float*>(static_cast<char*>(h->ws) + wp.head_scr);
  return FV_OK;
}

// the higher-order solvers' rows for a call whose scratch is `scr` (null under Euler, which takes none)
float* head_rk_rows(fv_handle* h, int B, float* scr) {
  return h->flow_solver != FV_FLOW_SOLVER_EULER ? scr + head_sampler_bytes(h, B) / sizeof(float) : nullptr;
}

// network evaluations of a sampler call, for the profiler's estimates: n_steps x the solver's stages
double flow_evals(const fv_handle* h, int n_steps) {
  static const int stages[4] = {1, 2, 2, 4};
  return (double)n_steps * stages[h->flow_solver];
}

// What the three sampler entry points (`who`) share, in the order of their checks: the handle, flow mode, own() -- the entry point's refusals for its mode
// and its pointers --, n_steps, B, own_late() -- its refusal of the shift --, the scratch (`too_small`: its message for a workspace bound for a smaller
// plan) and, inside the profiler's bracket, run(scratch, the solver's rows, stream) -- the entry point's one launcher call.  flops / bytes: the profiler's
// factors on evaluations x parameters (x B for the FLOPs)
template <class Own, class OwnLate, class Run>
int head_flow_sample_call(fv_handle* h, const char* who, int B, int n_steps, const char* too_small, double flops, double bytes, fv_stream s, Own&& own, OwnLate&& own_late,
                          Run&& run) {
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "%s: the head is not in flow mode (fv_head_set_flow)", who);
  FV_TRY(own());
  if (n_steps < 1) return fv_fail(FV_ERR_ARG, "%s: n_steps = %d must be >= 1", who, n_steps);
  if (B < 1 || B > h->d.max_batch) return fv_fail(FV_ERR_ARG, "%s: B=%d outside 1 .. max_batch=%d", who, B, h->d.max_batch);
  FV_TRY(own_late());
  float* scr = nullptr;
  FV_TRY(head_scratch(h, B, too_small, &scr));
  hipStream_t st = static_cast<hipStream_t>(s);
  const double work = flow_evals(h, n_steps) * head_param_count(h);
  prof_begin(h, FV_FAM_HEAD, flops * B * work, bytes * work, st);
  const int rc = run(scr, head_rk_rows(h, B, scr), st);
  prof_end(h, st);
  return rc;
}

// n host floats -> the handle's device vector *buf, allocated first when `fresh` (every setter has its own rule for that; an old vector stays until fv_destroy).
// A head kernel still in flight on any stream may be reading the previous values: a configuration call, so it simply waits
int head_upload(fv_handle* h, float** buf, bool fresh, const float* host, size_t n) {
  FV_HIP_CHECK(hipSetDevice(h->device));
  if (fresh) {
    void* p = nullptr;
    FV_TRY(dev_alloc(h, n * 4, &p));
    *buf = static_cast<float*>(p);
  }
  FV_HIP_CHECK(hipDeviceSynchronize());
  FV_HIP_CHECK(hipMemcpy(*buf, host, n * 4, hipMemcpyHostToDevice));
  return FV_OK;
}

}  // namespace

extern "C" {

int fv_head_layout(fv_handle* h, int64_t offsets[13]) {
  HandleScope _hs(h);
  if (!h || !offsets) return fv_fail(FV_ERR_ARG, "fv_head_layout: null argument");
  const fv::HeadOffsets ho = fv::head_offsets(h->hd);
  for (int i = 0; i <= fv::HP_TOTAL; ++i) offsets[i] = ho.o[i];
  return FV_OK;
}

int fv_head_saved_bytes(fv_handle* h, int B, size_t* out_bytes) {
  HandleScope _hs(h);
  if (!h || !out_bytes || B <= 0) return fv_fail(FV_ERR_ARG, "fv_head_saved_bytes: bad argument");
  *out_bytes = fv::head_saved_bytes(h->hd, B);
  return FV_OK;
}

int fv_head_forward(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B,
                    int training, float dropout_p, uint64_t seed, uint64_t offset, float* actions, void* saved,
                    fv_stream s) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  hipStream_t st = static_cast<hipStream_t>(s);
  prof_begin(h, FV_FAM_HEAD, 2.0 * B * head_param_count(h), 4.0 * head_param_count(h), st);
  const int rc = fv::launch_head_forward(h->hd, flat_params, pooled, states, B, training, dropout_p, seed, offset, actions,
                                         static_cast<float*>(saved), st, h->has_io ? &h->io : nullptr);
  prof_end(h, st);
  return rc;
}

int fv_head_set_io_norm(fv_handle* h, const float* state_mean, const float* state_std, const float* action_mean,
                        const float* action_std, float eps) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (!state_mean && !state_std && !action_mean && !action_std) { h->has_io = false; return FV_OK; }   // all NULL: folding off
  if (!state_mean || !state_std || !action_mean || !action_std) return fv_fail(FV_ERR_ARG, "fv_head_set_io_norm: give all four vectors or none");
  const int ds = h->hd.ds, da = h->hd.da;
  std::vector<float> v((size_t)2 * ds + 2 * da);
  for (int i = 0; i < ds; ++i) { v[i] = state_mean[i]; v[ds + i] = 1.0f / (state_std[i] + eps); }
  for (int i = 0; i < da; ++i) { v[2 * ds + i] = action_mean[i]; v[2 * ds + da + i] = action_std[i]; }
  FV_TRY(head_upload(h, &h->io_buf, !h->io_buf, v.data(), v.size()));   // allocated once: toggling the folding on / off / on does not grow the handle
  float* f = h->io_buf;
  h->io = fv::HeadIoNorm{f, f + ds, f + 2 * ds, f + 2 * ds + da};
  h->has_io = true;
  return FV_OK;
}

int fv_head_mse_backward(fv_handle* h, const float* flat_params, const float* actions, const float* targets, int B,
                         float dropout_p, const void* saved, float* loss, float* flat_grads, fv_stream s) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  float* scr = nullptr;
  FV_TRY(head_scratch(h, B, "workspace too small for head backward", &scr));
  hipStream_t st = static_cast<hipStream_t>(s);
  prof_begin(h, FV_FAM_HEAD, 4.0 * B * head_param_count(h), 8.0 * head_param_count(h), st);
  const int rc = fv::launch_head_backward(h->hd, flat_params, nullptr, actions, targets, B, dropout_p,
                                          static_cast<const float*>(saved), loss, flat_grads, scr, st, nullptr, 1.0f, &h->loss);
  prof_end(h, st);
  return rc;
}

int fv_head_set_flow(fv_handle* h, const fv_head_flow_spec* spec) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (spec) {
    if (spec->time_dim < 2 || spec->time_dim % 2) return fv_fail(FV_ERR_ARG, "fv_head_set_flow: time_dim = %d must be positive and even", spec->time_dim);
    if (!std::isfinite(spec->min_period) || !std::isfinite(spec->max_period) || !(spec->min_period > 0.f) || !(spec->max_period > spec->min_period))
      return fv_fail(FV_ERR_ARG, "fv_head_set_flow: periods must be finite with 0 < min_period < max_period (got %g, %g)", (double)spec->min_period, (double)spec->max_period);
    if (spec->time_dist != 0 && spec->time_dist != 1) return fv_fail(FV_ERR_ARG, "fv_head_set_flow: unknown time_dist %d (0 uniform, 1 logit-normal)", spec->time_dist);
    if (!std::isfinite(spec->dist_a) || !std::isfinite(spec->dist_b)) return fv_fail(FV_ERR_ARG, "fv_head_set_flow: dist_a / dist_b must be finite");
  }
  if (spec && h->hd.nb > 0) return fv_fail(FV_ERR_STATE, "fv_head_set_flow: the head is in bins mode (fv_head_set_bins); switch that off first");
  // the head's layout, the saved activations, the workspace plan and the training layouts all depend on the mode
  if (h->ws || h->train.ready || h->train.tower) return fv_fail(FV_ERR_STATE, "fv_head_set_flow: call it before fv_bind_workspace and before any fv_train_*_begin (sizes depend on the mode)");
  if (!spec) { h->hd.te = 0; h->hd.draws = 1; h->hd.pk = h->hd.pd = 0; h->flow_solver = FV_FLOW_SOLVER_EULER; h->flow_samples = 1; h->select_w = nullptr; h->flow = fv::HeadFlow{nullptr, 0, 0.f, 0.f}; h->guide = fv::HeadGuide{nullptr, 0, 0.f, 0}; return FV_OK; }
  const int half = spec->time_dim / 2;
  std::vector<float> fr(half);   // 2 pi / p_j, p_j geometric from min_period to max_period; in double, rounded once
  for (int j = 0; j < half; ++j) {
    const double frac = half > 1 ? (double)j / (half - 1) : 0.0;
    fr[j] = (float)(2.0 * 3.14159265358979323846 / ((double)spec->min_period * std::pow((double)spec->max_period / (double)spec->min_period, frac)));
  }
  const bool grow = h->flow_freq_cap < half;   // kept across off / on: toggling the mode, or asking for the same or a smaller time_dim, does not grow the handle (a LARGER one allocates anew)
  FV_TRY(head_upload(h, &h->flow_freq_buf, grow, fr.data(), (size_t)half));
  if (grow) h->flow_freq_cap = half;
  h->hd.te = spec->time_dim;
  h->flow = fv::HeadFlow{h->flow_freq_buf, spec->time_dist, spec->dist_a, spec->dist_b, h->hd.pk > 0 ? h->prefix_thr_buf : nullptr};
  return FV_OK;
}

int fv_head_set_bins(fv_handle* h, const fv_head_bins_spec* spec, const float* lo_host, const float* hi_host) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  const int da = h->hd.da;
  std::vector<float> tab;
  if (spec) {
    if (spec->bins < 2 || spec->bins > FV_HEAD_BINS_MAX) return fv_fail(FV_ERR_ARG, "fv_head_set_bins: bins = %d outside 2 .. %d", spec->bins, FV_HEAD_BINS_MAX);
    if (spec->decode != FV_BINS_DECODE_ARGMAX && spec->decode != FV_BINS_DECODE_MEAN) return fv_fail(FV_ERR_ARG, "fv_head_set_bins: unknown decode %d (0 argmax, 1 mean)", spec->decode);
    if (!std::isfinite(spec->sigma) || spec->sigma < 0.f) return fv_fail(FV_ERR_ARG, "fv_head_set_bins: sigma = %g must be finite and >= 0", (double)spec->sigma);
    if (spec->n_range < 1 || da % spec->n_range) return fv_fail(FV_ERR_ARG, "fv_head_set_bins: n_range = %d must be >= 1 and divide action_dim = %d", spec->n_range, da);
    if (!lo_host || !hi_host) return fv_fail(FV_ERR_ARG, "fv_head_set_bins: null range");
    if ((int64_t)da * spec->bins > FV_HEAD_BINS_MAX_WIDTH)
      return fv_fail(FV_ERR_ARG, "fv_head_set_bins: action_dim * bins = %d * %d exceeds %d (the head's linear kernels take one output per block row)", da, spec->bins, FV_HEAD_BINS_MAX_WIDTH);
    tab.resize((size_t)3 * spec->n_range);   // [lo | hi | w]; w in double, rounded once
    for (int i = 0; i < spec->n_range; ++i) {
      const float lo = lo_host[i], hi = hi_host[i];
      const float w = (float)(((double)hi - (double)lo) / spec->bins);
      if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !std::isfinite(w) || !(w > 0.f))
        return fv_fail(FV_ERR_ARG, "fv_head_set_bins: range %d = [%g, %g] must be finite with lo < hi", i, (double)lo, (double)hi);
      tab[i] = lo; tab[spec->n_range + i] = hi; tab[2 * spec->n_range + i] = w;
    }
  }
  // the head's layout, the saved activations, the workspace plan and the training layouts all depend on the mode
  if (h->ws || h->train.ready || h->train.tower) return fv_fail(FV_ERR_STATE, "fv_head_set_bins: call it before fv_bind_workspace and before any fv_train_*_begin (sizes depend on the mode)");
  if (!spec) { h->hd.nb = 0; h->hd.bn = nullptr; h->bins = fv::HeadBins{nullptr, 0, 0.f, 0}; return FV_OK; }
  if (h->hd.te > 0) return fv_fail(FV_ERR_STATE, "fv_head_set_bins: the head is in flow mode (fv_head_set_flow); switch that off first");
  const bool grow = h->bins_range_cap < spec->n_range;   // (kept across off / on: toggling the mode does not grow the handle)
  FV_TRY(head_upload(h, &h->bins_range_buf, grow, tab.data(), tab.size()));
  if (grow) h->bins_range_cap = spec->n_range;
  h->bins = fv::HeadBins{h->bins_range_buf, spec->n_range, spec->sigma, spec->decode};
  h->hd.nb = spec->bins;
  h->hd.bn = &h->bins;
  return FV_OK;
}

int fv_head_bins_logits(fv_handle* h, const void* saved, int B, const float** logits_dev) {
  HandleScope _hs(h);
  if (!h || !saved || !logits_dev || B < 1) return fv_fail(FV_ERR_ARG, "fv_head_bins_logits: bad argument");
  if (h->hd.nb <= 0) return fv_fail(FV_ERR_STATE, "fv_head_bins_logits: the head is not in bins mode (fv_head_set_bins)");
  *logits_dev = fv::head_saved_logits(h->hd, B, static_cast<float*>(const_cast<void*>(saved)));
  return FV_OK;
}

int fv_head_bins_probs(fv_handle* h, const void* saved, int B, float* probs_dev, fv_stream s) {
  HandleScope _hs(h);
  if (!h || !saved || !probs_dev || B < 1) return fv_fail(FV_ERR_ARG, "fv_head_bins_probs: bad argument");
  if (h->hd.nb <= 0) return fv_fail(FV_ERR_STATE, "fv_head_bins_probs: the head is not in bins mode (fv_head_set_bins)");
  const float* logits = fv::head_saved_logits(h->hd, B, static_cast<float*>(const_cast<void*>(saved)));
  return fv::launch_bins_decode(h->bins, logits, nullptr, probs_dev, (long)B * h->hd.da, h->hd.nb, h->hd.da, nullptr, nullptr, static_cast<hipStream_t>(s));
}

int fv_head_set_flow_prefix(fv_handle* h, int chunk, int max_delay, const uint32_t* thresholds_host) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_set_flow_prefix: the head is not in flow mode (fv_head_set_flow)");
  // fusion.0's width, the saved activations, the workspace plan and the training layouts all depend on the mode
  if (h->ws || h->train.ready || h->train.tower)
    return fv_fail(FV_ERR_STATE, "fv_head_set_flow_prefix: call it before fv_bind_workspace and before any fv_train_*_begin (sizes depend on the mode)");
  if (!thresholds_host) { h->hd.pk = h->hd.pd = 0; h->flow.thr = nullptr; return FV_OK; }
  if (chunk < 2 || h->hd.da % chunk) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_prefix: chunk=%d must be >= 2 and divide action_dim=%d", chunk, h->hd.da);
  if (max_delay < 1 || max_delay > chunk - 1) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_prefix: max_delay=%d outside 1 .. chunk - 1 = %d", max_delay, chunk - 1);
  for (int j = 0; j <= max_delay; ++j)
    if (thresholds_host[j] > (1u << 24) || (j > 0 && thresholds_host[j] < thresholds_host[j - 1]))
      return fv_fail(FV_ERR_ARG, "fv_head_set_flow_prefix: thresholds must be non-decreasing and at most 2^24 (entry %d = %u)", j, thresholds_host[j]);
  if (thresholds_host[max_delay] != (1u << 24)) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_prefix: the last threshold must be 2^24, got %u", thresholds_host[max_delay]);
  const bool grow = h->prefix_thr_cap < max_delay + 1;   // (a longer table allocates anew; toggling the mode does not grow the handle)
  static_assert(sizeof(uint32_t) == sizeof(float), "head_upload copies 4-byte words");
  FV_TRY(head_upload(h, reinterpret_cast<float**>(&h->prefix_thr_buf), grow, reinterpret_cast<const float*>(thresholds_host), (size_t)max_delay + 1));
  if (grow) h->prefix_thr_cap = max_delay + 1;
  h->hd.pk = chunk;
  h->hd.pd = max_delay;
  h->flow.thr = h->prefix_thr_buf;
  return FV_OK;
}

int fv_head_set_flow_draws(fv_handle* h, int draws) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_set_flow_draws: the head is not in flow mode (fv_head_set_flow)");
  // the saved activations, the backward's scratch, the workspace plan and the training plan all depend on it
  if (h->ws || h->train.ready || h->train.tower) return fv_fail(FV_ERR_STATE, "fv_head_set_flow_draws: call it before fv_bind_workspace and before any fv_train_*_begin (sizes depend on it)");
  if (draws < 1 || draws > FV_FLOW_DRAWS_MAX) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_draws: draws = %d outside 1 .. %d", draws, FV_FLOW_DRAWS_MAX);
  h->hd.draws = draws;
  return FV_OK;
}

int fv_head_set_flow_time(fv_handle* h, const fv_head_flow_time_spec* spec) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_set_flow_time: the head is not in flow mode (fv_head_set_flow)");
  if (!spec) { h->flow.tm = fv::FlowTime{}; return FV_OK; }
  if (spec->dist < 0 || spec->dist > 2) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_time: unknown dist %d (0 uniform, 1 logit-normal, 2 Beta)", spec->dist);
  if (!std::isfinite(spec->a) || !std::isfinite(spec->b) || !std::isfinite(spec->t_lo) || !std::isfinite(spec->t_hi))
    return fv_fail(FV_ERR_ARG, "fv_head_set_flow_time: a, b, t_lo and t_hi must be finite");
  if (spec->dist == 2 && (spec->a < 0.25f || spec->a > 32.f || spec->b < 0.25f || spec->b > 32.f))
    return fv_fail(FV_ERR_ARG, "fv_head_set_flow_time: Beta(%g, %g) outside [0.25, 32] (the range the inversion is held to)", (double)spec->a, (double)spec->b);
  if (!(spec->t_lo >= 0.f && spec->t_lo < spec->t_hi && spec->t_hi <= 1.f))
    return fv_fail(FV_ERR_ARG, "fv_head_set_flow_time: the range must be 0 <= t_lo < t_hi <= 1 (got %g, %g)", (double)spec->t_lo, (double)spec->t_hi);
  if (spec->stratify != 0 && spec->stratify != 1) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_time: stratify = %d must be 0 or 1", spec->stratify);
  fv::FlowTime tm;
  tm.on = 1; tm.dist = spec->dist; tm.stratify = spec->stratify; tm.a = spec->a; tm.b = spec->b; tm.t_lo = spec->t_lo; tm.t_hi = spec->t_hi;
  if (spec->dist == 2) tm.lbeta = std::lgamma((double)spec->a) + std::lgamma((double)spec->b) - std::lgamma((double)spec->a + (double)spec->b);
  h->flow.tm = tm;
  return FV_OK;
}

int fv_head_flow_prepare(fv_handle* h, const float* targets, int B, uint64_t seed, uint64_t offset, const float* noise, const float* t, void* saved,
                         float* u_out, fv_stream s) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_flow_prepare: the head is not in flow mode (fv_head_set_flow)");
  return fv::launch_flow_prepare(h->hd, h->flow, targets, B, seed, offset, noise, t, static_cast<float*>(saved), u_out, static_cast<hipStream_t>(s));
}

int fv_head_flow_prepare_prefix(fv_handle* h, const float* targets, int B, uint64_t seed, uint64_t offset, const float* noise, const float* t, const int32_t* delays,
                                void* saved, float* u_out, fv_stream s) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_flow_prepare_prefix: the head is not in flow mode (fv_head_set_flow)");
  if (h->hd.pk <= 0) return fv_fail(FV_ERR_STATE, "fv_head_flow_prepare_prefix: prefix mode is off (fv_head_set_flow_prefix)");
  if (!delays) return fv_fail(FV_ERR_ARG, "fv_head_flow_prepare_prefix: null delays (fv_head_flow_prepare draws them)");
  return fv::launch_flow_prepare(h->hd, h->flow, targets, B, seed, offset, noise, t, static_cast<float*>(saved), u_out, static_cast<hipStream_t>(s), delays);
}

int fv_head_flow_sample(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                        uint64_t seed, uint64_t offset, float* actions, fv_stream s) {
  HandleScope _hs(h);
  return head_flow_sample_call(
      h, "fv_head_flow_sample", B, n_steps, "workspace too small for the flow sampler", 2.0, 4.0, s,
      [&] { return !flat_params || !pooled || !states || !actions ? fv_fail(FV_ERR_ARG, "fv_head_flow_sample: null pointer") : FV_OK; }, [] { return (int)FV_OK; },
      [&](float* scr, float* rk_rows, hipStream_t st) {
        return fv::launch_flow_sample(h->hd, h->flow, flat_params, pooled, states, B, n_steps, noise, seed, offset, actions, scr, st, h->has_io ? &h->io : nullptr, h->flow_solver,
                                      rk_rows);
      });
}

int fv_head_flow_sample_prefix(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                               uint64_t seed, uint64_t offset, const float* prev, int shift, const int32_t* delays, float* actions, float* chunk_out,
                               fv_stream s) {
  HandleScope _hs(h);
  return head_flow_sample_call(
      h, "fv_head_flow_sample_prefix", B, n_steps, "workspace too small for the flow sampler", 2.0, 4.0, s,
      [&] {
        if (h->hd.pk <= 0) return fv_fail(FV_ERR_STATE, "fv_head_flow_sample_prefix: prefix mode is off (fv_head_set_flow_prefix)");
        return !flat_params || !pooled || !states || !prev || !delays || !actions ? fv_fail(FV_ERR_ARG, "fv_head_flow_sample_prefix: null pointer") : FV_OK;
      },
      [&] { return shift < 0 || shift > h->hd.pk ? fv_fail(FV_ERR_ARG, "fv_head_flow_sample_prefix: shift = %d outside 0 .. chunk = %d", shift, h->hd.pk) : FV_OK; },
      [&](float* scr, float* rk_rows, hipStream_t st) {
        const fv::FlowPin pin{prev, delays, shift, chunk_out};
        return fv::launch_flow_sample(h->hd, h->flow, flat_params, pooled, states, B, n_steps, noise, seed, offset, actions, scr, st, h->has_io ? &h->io : nullptr, h->flow_solver,
                                      rk_rows, &pin);
      });
}

int fv_head_set_flow_solver(fv_handle* h, int solver) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_set_flow_solver: the head is not in flow mode (fv_head_set_flow)");
  if (solver < FV_FLOW_SOLVER_EULER || solver > FV_FLOW_SOLVER_RK4)
    return fv_fail(FV_ERR_ARG, "fv_head_set_flow_solver: unknown solver %d (0 Euler, 1 midpoint, 2 Heun, 3 RK4)", solver);
  // the step's start and the running stage sum, two (B, action_dim) rows, join the plan with the first call that names a higher-order solver: a workspace
  // bound before that does not hold them
  if (solver != FV_FLOW_SOLVER_EULER && !h->flow_rk_rows) {
    if (h->ws) return fv_fail(FV_ERR_STATE, "fv_head_set_flow_solver: the first call for a higher-order solver must come before fv_bind_workspace (the workspace grows by two rows)");
    h->flow_rk_rows = true;
  }
  h->flow_solver = solver;
  return FV_OK;
}

int fv_head_set_flow_guidance(fv_handle* h, int chunk, const float* step_weights_host, float max_guidance_weight) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_set_flow_guidance: the head is not in flow mode (fv_head_set_flow)");
  if (!step_weights_host) { h->guide = fv::HeadGuide{nullptr, 0, 0.f, 0}; return FV_OK; }
  if (chunk < 1 || h->hd.da % chunk) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_guidance: chunk=%d must be >= 1 and divide action_dim=%d", chunk, h->hd.da);
  int live = 0;
  for (int k = 0; k < chunk; ++k) {
    if (!std::isfinite(step_weights_host[k]) || step_weights_host[k] < 0.f)
      return fv_fail(FV_ERR_ARG, "fv_head_set_flow_guidance: step weight %d = %g must be finite and >= 0", k, (double)step_weights_host[k]);
    if (step_weights_host[k] != 0.f) live = k + 1;
  }
  if (!std::isfinite(max_guidance_weight) || !(max_guidance_weight > 0.f))
    return fv_fail(FV_ERR_ARG, "fv_head_set_flow_guidance: max_guidance_weight = %g must be finite and > 0", (double)max_guidance_weight);
  // the guided sampler's rows (the unguided sampler's and the backward chain's partial sums on top) are larger than the head part of the plan without
  // them, and they join the plan with the first configuration: a workspace bound before that does not hold them
  if (h->ws && h->guide_chunk == 0)
    return fv_fail(FV_ERR_STATE, "fv_head_set_flow_guidance: the first call must come before fv_bind_workspace (the workspace grows by the guided sampler's rows)");
  FV_TRY(head_upload(h, &h->guide_buf, h->guide_chunk != chunk, step_weights_host, (size_t)chunk));   // (another chunk length allocates anew)
  h->guide_chunk = chunk;
  h->guide = fv::HeadGuide{h->guide_buf, chunk, max_guidance_weight, live};
  return FV_OK;
}

int fv_head_flow_sample_guided(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                               uint64_t seed, uint64_t offset, const float* prev, int shift, const int32_t* row_mask, float* actions, float* chunk_out,
                               fv_stream s) {
  HandleScope _hs(h);
  return head_flow_sample_call(
      h, "fv_head_flow_sample_guided", B, n_steps, "workspace too small for the guided flow sampler", 4.0, 8.0, s,
      [&] {
        if (!h->guide.step_w) return fv_fail(FV_ERR_STATE, "fv_head_flow_sample_guided: guidance is not configured (fv_head_set_flow_guidance)");
        return !flat_params || !pooled || !states || !prev || !actions ? fv_fail(FV_ERR_ARG, "fv_head_flow_sample_guided: null pointer") : FV_OK;
      },
      [&] { return shift < 0 || shift > h->guide.chunk ? fv_fail(FV_ERR_ARG, "fv_head_flow_sample_guided: shift = %d outside 0 .. chunk = %d", shift, h->guide.chunk) : FV_OK; },
      [&](float* scr, float* rk_rows, hipStream_t st) {
        return fv::launch_flow_sample_guided(h->hd, h->flow, h->guide, flat_params, pooled, states, B, n_steps, noise, seed, offset, prev, shift, row_mask, actions, chunk_out, scr,
                                             st, h->has_io ? &h->io : nullptr, h->flow_solver, rk_rows);
      });
}

int fv_head_set_flow_samples(fv_handle* h, int max_samples, int chunk, const float* step_weights_host) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_set_flow_samples: the head is not in flow mode (fv_head_set_flow)");
  if (max_samples < 1 || max_samples > FV_FLOW_SAMPLES_MAX) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_samples: max_samples = %d outside 1 .. %d", max_samples, FV_FLOW_SAMPLES_MAX);
  if (step_weights_host) {
    if (chunk < 1 || h->hd.da % chunk) return fv_fail(FV_ERR_ARG, "fv_head_set_flow_samples: chunk=%d must be >= 1 and divide action_dim=%d", chunk, h->hd.da);
    for (int k = 0; k < chunk; ++k)
      if (!std::isfinite(step_weights_host[k]) || step_weights_host[k] < 0.f)
        return fv_fail(FV_ERR_ARG, "fv_head_set_flow_samples: step weight %d = %g must be finite and >= 0", k, (double)step_weights_host[k]);
  }
  // the sampler's rows (and the higher-order solvers' two) are sized for max_samples x B head rows: a workspace bound for another count does not fit
  if (max_samples != h->flow_samples && h->ws)
    return fv_fail(FV_ERR_STATE, "fv_head_set_flow_samples: the call that changes max_samples must come before fv_bind_workspace (the sampler's rows grow with it)");
  if (step_weights_host) {
    FV_TRY(head_upload(h, &h->select_w_buf, h->select_chunk != chunk, step_weights_host, (size_t)chunk));   // (another chunk length allocates anew)
    h->select_chunk = chunk;
  }
  h->select_w = step_weights_host ? h->select_w_buf : nullptr;
  h->flow_samples = max_samples;
  return FV_OK;
}

int fv_head_flow_sample_multi(fv_handle* h, const float* flat_params, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                              uint64_t seed, uint64_t offset, int S, int select, const float* prev, int shift, const int32_t* row_mask, const int32_t* delays,
                              float* actions, float* chunk_out, float* candidates_out, int32_t* choice_out, float* scores_out, float* spread_out, fv_stream s) {
  HandleScope _hs(h);
  const bool coherent = select == FV_FLOW_SELECT_COHERENT;
  return head_flow_sample_call(
      h, "fv_head_flow_sample_multi", B, n_steps, "workspace too small for the flow sampler's candidates", 2.0 * S, 4.0, s,
      [&] {
        if (delays && h->hd.pk <= 0) return fv_fail(FV_ERR_STATE, "fv_head_flow_sample_multi: delays need prefix mode (fv_head_set_flow_prefix)");
        if (coherent && !h->select_w) return fv_fail(FV_ERR_STATE, "fv_head_flow_sample_multi: coherent selection has no step weights (fv_head_set_flow_samples)");
        if (!flat_params || !pooled || !states || !actions || !chunk_out || ((delays || coherent) && !prev)) return fv_fail(FV_ERR_ARG, "fv_head_flow_sample_multi: null pointer");
        if (S < 1 || S > h->flow_samples) return fv_fail(FV_ERR_ARG, "fv_head_flow_sample_multi: S = %d outside 1 .. max_samples = %d (fv_head_set_flow_samples)", S, h->flow_samples);
        if (select != FV_FLOW_SELECT_FIRST && select != FV_FLOW_SELECT_MEDOID && !coherent)
          return fv_fail(FV_ERR_ARG, "fv_head_flow_sample_multi: unknown select %d (0 first, 1 medoid, 2 coherent)", select);
        if (S > 1 && (offset >> 56 & 15))
          return fv_fail(FV_ERR_ARG, "fv_head_flow_sample_multi: bits 56 .. 59 of the offset number the candidates and must be 0 with more than one");
        return (int)FV_OK;
      },
      [&] {
        if (delays && (shift < 0 || shift > h->hd.pk)) return fv_fail(FV_ERR_ARG, "fv_head_flow_sample_multi: shift = %d outside 0 .. chunk = %d", shift, h->hd.pk);
        if (coherent && (shift < 0 || shift > h->select_chunk)) return fv_fail(FV_ERR_ARG, "fv_head_flow_sample_multi: shift = %d outside 0 .. chunk = %d", shift, h->select_chunk);
        return (int)FV_OK;
      },
      [&](float* scr, float* rk_rows, hipStream_t st) {
        const fv::FlowPin pin{prev, delays, shift, nullptr};
        const fv::FlowSelect sel{select, prev, shift, row_mask, h->select_w, h->select_chunk, actions, chunk_out, candidates_out, choice_out, scores_out, spread_out};
        return fv::launch_flow_sample_multi(h->hd, h->flow, flat_params, pooled, states, B, S, n_steps, noise, seed, offset, scr, st, h->has_io ? &h->io : nullptr, h->flow_solver,
                                            rk_rows, delays ? &pin : nullptr, sel);
      });
}

int fv_head_set_loss(fv_handle* h, const fv_head_loss_spec* spec) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  // another chunk length: the weight vectors' sizes no longer fit, so weighting is off until fv_head_set_loss_weights runs again
  if (!spec) {
    if (h->loss.chunk != 1) h->loss.dim_w = h->loss.step_w = nullptr;
    h->loss.kind = FV_LOSS_MSE; h->loss.beta = 1.0f; h->loss.chunk = 1;
    return FV_OK;
  }
  if (spec->kind != FV_LOSS_MSE && spec->kind != FV_LOSS_L1 && spec->kind != FV_LOSS_SMOOTH_L1) return fv_fail(FV_ERR_ARG, "fv_head_set_loss: unknown loss kind %d", spec->kind);
  if (spec->kind == FV_LOSS_SMOOTH_L1 && !(spec->beta > 0.f && std::isfinite(spec->beta))) return fv_fail(FV_ERR_ARG, "fv_head_set_loss: smooth-L1 beta must be positive and finite");
  if (spec->chunk < 1 || h->hd.da % spec->chunk) return fv_fail(FV_ERR_ARG, "fv_head_set_loss: chunk=%d must be >= 1 and divide action_dim=%d", spec->chunk, h->hd.da);
  if (spec->chunk != h->loss.chunk) h->loss.dim_w = h->loss.step_w = nullptr;
  h->loss.kind = spec->kind;
  h->loss.beta = spec->kind == FV_LOSS_SMOOTH_L1 ? spec->beta : 1.0f;
  h->loss.chunk = spec->chunk;
  return FV_OK;
}

int fv_head_set_loss_mask(fv_handle* h, const uint8_t* pad_dev) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  h->loss.pad = pad_dev;
  return FV_OK;
}

int fv_head_set_loss_weights(fv_handle* h, const float* dim_w, const float* step_w) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "null handle");
  if (!dim_w && !step_w) { h->loss.dim_w = h->loss.step_w = nullptr; return FV_OK; }   // both NULL: weighting off
  const int da = h->hd.da, K = h->loss.chunk, A = da / K;
  for (int i = 0; dim_w && i < A; ++i)
    if (!(dim_w[i] >= 0.f) || !std::isfinite(dim_w[i])) return fv_fail(FV_ERR_ARG, "fv_head_set_loss_weights: dim_w[%d] = %g must be finite and >= 0", i, (double)dim_w[i]);
  for (int k = 0; step_w && k < K; ++k)
    if (!(step_w[k] >= 0.f) || !std::isfinite(step_w[k])) return fv_fail(FV_ERR_ARG, "fv_head_set_loss_weights: step_w[%d] = %g must be finite and >= 0", k, (double)step_w[k]);
  std::vector<float> v((size_t)2 * da, 1.0f);   // a NULL vector: ones
  for (int i = 0; dim_w && i < A; ++i) v[i] = dim_w[i];
  for (int k = 0; step_w && k < K; ++k) v[da + k] = step_w[k];
  FV_TRY(head_upload(h, &h->loss_w, !h->loss_w, v.data(), v.size()));   // allocated once, sized for every chunk length that divides action_dim
  h->loss.dim_w = h->loss_w;
  h->loss.step_w = h->loss_w + da;
  return FV_OK;
}

int fv_head_loss_per_dim(fv_handle* h, const float* actions, const float* targets, int B, float* out_dev, fv_stream s) {
  HandleScope _hs(h);
  if (!h || !actions || !targets || !out_dev) return fv_fail(FV_ERR_ARG, "fv_head_loss_per_dim: null argument");
  if (B < 1) return fv_fail(FV_ERR_ARG, "fv_head_loss_per_dim: B must be positive");
  // (draws: actions and targets have S B rows, the mask keeps B)
  return fv::launch_loss_per_dim(actions, targets, h->loss.pad, out_dev, (long)fv::head_rows(h->hd, B) * h->loss.chunk, h->hd.da / h->loss.chunk, static_cast<hipStream_t>(s),
                                 (long)B * h->loss.chunk);
}

int fv_head_loss_per_time(fv_handle* h, const float* actions, const float* targets, const float* t, int B, int n_buckets, float* out_dev, fv_stream s) {
  HandleScope _hs(h);
  if (!h || !actions || !targets || !t || !out_dev) return fv_fail(FV_ERR_ARG, "fv_head_loss_per_time: null argument");
  if (h->hd.te <= 0) return fv_fail(FV_ERR_STATE, "fv_head_loss_per_time: the head is not in flow mode (fv_head_set_flow)");
  if (B < 1) return fv_fail(FV_ERR_ARG, "fv_head_loss_per_time: B must be positive");
  if (n_buckets < 1 || n_buckets > FV_LOSS_TIME_BUCKETS_MAX)
    return fv_fail(FV_ERR_ARG, "fv_head_loss_per_time: n_buckets = %d outside 1 .. %d", n_buckets, FV_LOSS_TIME_BUCKETS_MAX);
  // (draws: actions, targets and t have S B rows, the mask keeps B)
  return fv::launch_loss_per_time(actions, targets, t, h->loss.pad, out_dev, fv::head_rows(h->hd, B), B, h->hd.da, h->loss.chunk, n_buckets, static_cast<hipStream_t>(s));
}

int fv_head_loss_metrics(fv_handle* h, const float** dev) {
  HandleScope _hs(h);
  if (!h || !dev) return fv_fail(FV_ERR_ARG, "fv_head_loss_metrics: null argument");
  *dev = h->loss.metrics;
  return FV_OK;
}

int fv_head_backward(fv_handle* h, const float* flat_params, const float* grad_actions, int B, float dropout_p,
                     const void* saved, float* flat_grads, fv_stream s) {
  HandleScope _hs(h);
  if (!h || !grad_actions) return fv_fail(FV_ERR_ARG, "fv_head_backward: null argument");
  if (h->hd.nb > 0) return fv_fail(FV_ERR_STATE, "fv_head_backward: a bins head trains through its own loss (fv_head_mse_backward); the decode is not differentiated");
  float* scr = nullptr;
  FV_TRY(head_scratch(h, B, "workspace too small for head backward", &scr));
  return fv::launch_head_backward(h->hd, flat_params, grad_actions, nullptr, nullptr, B, dropout_p,
                                  static_cast<const float*>(saved), nullptr, flat_grads, scr, static_cast<hipStream_t>(s));
}

// ---- temporal ensembling of action chunks (csrc/chunk_kernels.hip ensemble_step_kernel)
struct fv_ensembler {
  int n_env = 0, K = 0, A = 0;
  int head = 0;              // ring position: the slot of the time step served next (host state, a kernel argument)
  void* dev = nullptr;       // ONE allocation: ens | count | w | cw
  float* ens = nullptr;
  int32_t* count = nullptr;
  const float *w = nullptr, *cw = nullptr;
};

int fv_ensemble_create(fv_handle* h, int n_env, int chunk, int step_dim, float coeff, fv_ensembler** out) {
  HandleScope _hs(h);
  if (!h || !out) return fv_fail(FV_ERR_ARG, "fv_ensemble_create: null argument");
  *out = nullptr;
  if (n_env < 1 || chunk < 1 || step_dim < 1) return fv_fail(FV_ERR_ARG, "fv_ensemble_create: n_env = %d, chunk = %d, step_dim = %d must all be >= 1", n_env, chunk, step_dim);
  if (!std::isfinite(coeff)) return fv_fail(FV_ERR_ARG, "fv_ensemble_create: coeff must be finite");
  const size_t slots = (size_t)n_env * chunk;
  if (slots * step_dim > ((size_t)1 << 40)) return fv_fail(FV_ERR_ARG, "fv_ensemble_create: n_env * chunk * step_dim is more than 2^40");
  // the tables in double, rounded once: w[i] = exp(-coeff i), cw[i] = w[0] + .. + w[i]
  std::vector<float> tab;
  try {
    tab.resize((size_t)2 * chunk);
  } catch (const std::exception&) {
    return fv_fail(FV_ERR_STATE, "fv_ensemble_create: out of host memory");
  }
  double run = 0.0;
  for (int i = 0; i < chunk; ++i) {
    const double wi = std::exp(-(double)coeff * i);
    run += wi;
    tab[i] = (float)wi;
    tab[chunk + i] = (float)run;
    if (!std::isfinite(tab[chunk + i]) || !(tab[chunk + i] > 0.f))
      return fv_fail(FV_ERR_ARG, "fv_ensemble_create: coeff = %g over %d steps leaves the fp32 range", (double)coeff, chunk);
  }
  FV_HIP_CHECK(hipSetDevice(h->device));
  const size_t ens_bytes = align_up(slots * step_dim * sizeof(float)), cnt_bytes = align_up(slots * sizeof(int32_t)), tab_bytes = align_up(tab.size() * sizeof(float));
  void* dev = nullptr;
  FV_HIP_CHECK(hipMalloc(&dev, ens_bytes + cnt_bytes + tab_bytes));
  char* base = static_cast<char*>(dev);
  hipError_t e = hipMemset(base, 0, ens_bytes + cnt_bytes);
  if (e == hipSuccess) e = hipMemcpy(base + ens_bytes + cnt_bytes, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { (void)hipFree(dev); return fv_hip_fail(e, "fv_ensemble_create: upload"); }
  fv_ensembler* en = new (std::nothrow) fv_ensembler;
  if (!en) { (void)hipFree(dev); return fv_fail(FV_ERR_STATE, "fv_ensemble_create: out of host memory"); }
  en->n_env = n_env; en->K = chunk; en->A = step_dim; en->dev = dev;
  en->ens = reinterpret_cast<float*>(base);
  en->count = reinterpret_cast<int32_t*>(base + ens_bytes);
  en->w = reinterpret_cast<const float*>(base + ens_bytes + cnt_bytes);
  en->cw = en->w + chunk;
  *out = en;
  return FV_OK;
}

int fv_ensemble_destroy(fv_handle* h, fv_ensembler* e) {
  HandleScope _hs(h);
  if (!h) return fv_fail(FV_ERR_ARG, "fv_ensemble_destroy: null handle");
  if (!e) return FV_OK;
  FV_HIP_CHECK(hipSetDevice(h->device));
  const hipError_t err = hipFree(e->dev);    // (waits for a step still in flight on the ring)
  delete e;
  if (err != hipSuccess) return fv_hip_fail(err, "fv_ensemble_destroy: hipFree");
  return FV_OK;
}

int fv_ensemble_reset(fv_handle* h, fv_ensembler* e, int env, fv_stream s) {
  HandleScope _hs(h);
  if (!h || !e) return fv_fail(FV_ERR_ARG, "fv_ensemble_reset: null argument");
  if (env < -1 || env >= e->n_env) return fv_fail(FV_ERR_ARG, "fv_ensemble_reset: env = %d outside -1 .. %d", env, e->n_env - 1);
  // the counts alone carry the history: a slot with count 0 takes the next chunk's row as it is.  Stream-ordered, no host synchronisation
  int32_t* at = env < 0 ? e->count : e->count + (size_t)env * e->K;
  const size_t n = (env < 0 ? (size_t)e->n_env : 1) * e->K;
  FV_HIP_CHECK(hipMemsetAsync(at, 0, n * sizeof(int32_t), static_cast<hipStream_t>(s)));
  return FV_OK;
}

int fv_ensemble_step(fv_handle* h, fv_ensembler* e, const float* chunks, float* actions, fv_stream s) {
  HandleScope _hs(h);
  if (!h || !e || !chunks || !actions) return fv_fail(FV_ERR_ARG, "fv_ensemble_step: null argument");
  const int rc = fv::launch_ensemble_step(chunks, e->ens, e->count, actions, e->w, e->cw, e->n_env, e->K, e->A, e->head, static_cast<hipStream_t>(s));
  if (rc != FV_OK) return rc;
  e->head = (e->head + 1) % e->K;
  return FV_OK;
}
}  // extern "C"
