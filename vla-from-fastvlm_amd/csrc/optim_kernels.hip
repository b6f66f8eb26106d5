// optim_kernels.hip -- the fused global-norm clip + AdamW step on one flat buffer, in its two forms, and axpy.  Both forms evaluate common.h's adamw_update /
// ema_update per element, so a grouped step whose groups all carry lr_scale 1 and one decay gives the single-group step's bits.
//   single group (fv_adamw_clip_step[_ema]): sumsq_kernel + its fold, adamw_kernel<EMA>   trainer.py:60-66,178-180; lerobot configuration_fastvla.py:51-55
//   axpy_kernel: gradient accumulation over micro-batches / an upstream loss gradient
//   PARAMETER GROUPS (fv_adamw_clip_step_groups): per group a learning-rate factor, a weight decay and a frozen flag; one global clip norm over the non-frozen
//   elements, and a gradient norm per group.
//   torch.optim.AdamW's param_groups + clip_grad_norm_ over the parameters with requires_grad (the reference's step body, training/trainer.py:60-66,178-180,
//   knows one group only: it trains a 3 M-parameter head).
// The table (kernels.h AdamwGroupsTable) is built once on the host: every group cut into segments of <= FV_ADAMW_SEGMENT floats, all boundaries multiples of
// 4 floats -- so every access below is a 16-byte one, a block reads its group's settings once (no per-element search) and a frozen segment's block leaves
// before it has touched p, g, m or v.  Both kernels over the data move what adamw_kernel / sumsq_kernel move: 4 + 28 bytes per element (4 + 36 in the EMA
// instance of the step, fv_adamw_clip_step_ema, which keeps the average e of p in the same pass).
//   STEP GUARD (fv_step_guard, fv_adamw_clip_step_guarded): between the norm and the step ONE one-block decision launch -- non-finite norm, or a saturation flag
//   above the floor of the dynamic loss scale: skip, back the scale off; otherwise apply, grow it after growth_interval good steps -- and the GUARD instances of
//   both step kernels, which read that decision once per block: an early return on a skip, coef and the reported norms times 1 / delta (a power of two) otherwise.
// Summation order is fixed (per-thread strided sums, wave butterfly, four wave sums added pairwise): no float atomics, two runs give the same bits.
#include "kernels.h"

namespace fv {
namespace {

// ---- the single-group step ----
// Global gradient norm in a FIXED summation order (per-block partials, then one block folds them): float atomics would make
// the norm -- and through the clip coefficient every parameter -- depend on arrival order, so two data-parallel replicas
// (or two runs) would drift apart by an ulp per step.
constexpr int SUMSQ_BLOCKS = 1024;
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, float* __restrict__ partial) {
  __shared__ float red[4];
  // 16-byte loads, four independent sums per thread (the unfrozen path's 2 GB gradient: 0.84 -> ~0.45 ms); a fixed order either way
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 v = g4[i];
    s0 += v.x * v.x; s1 += v.y * v.y; s2 += v.z * v.z; s3 += v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) { const float v = g[(n4 << 2) + threadIdx.x]; s0 += v * v; }
  float s = wave_sum((s0 + s1) + (s2 + s3));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[1 + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void sumsq_fold_kernel(float* __restrict__ partial, int nb) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += partial[1 + i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// EMA instance (fv_adamw_clip_step_ema): also e <- ema_update(e, p_new, ema_w) while p_new is in its register, 8 more bytes per element.  The plain instance
// never looks at e / ema_w: it is the kernel as it was.
// GUARD instances (fv_adamw_clip_step_guarded): every block reads the decision step_guard_decide_kernel left in the guard's block -- one scalar load, nothing per
// element.  Skip: the norm is still reported, then the block leaves before it touches p, m, v or e.  Apply: coef and the reported norms times the decision's
// 1 / delta, an exact power of two, so the step has the bits of the plain step over gradients that never carried delta.  The plain instances never look at `gd`.
template <bool EMA, bool GUARD>
__device__ __forceinline__ void adamw_body(float* __restrict__ p, const float* __restrict__ g,
                                           float* __restrict__ m, float* __restrict__ v, long n,
                                           const fv_adamw_hparams& hp, float bc1, float bc2_sqrt,
                                           const float* __restrict__ sumsq, float* __restrict__ norm_out,
                                           float* __restrict__ e, float ema_w, const GuardWords* __restrict__ gd) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  // torch clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max = 1)
  float norm = sqrtf(*sumsq) * hp.grad_scale;
  if constexpr (GUARD) norm *= gd->inv_delta;
  float coef = hp.grad_scale;
  if (hp.max_grad_norm > 0.f) coef *= fminf(hp.max_grad_norm / (norm + 1e-6f), 1.0f);
  if constexpr (GUARD) coef *= gd->inv_delta;
  if (i == 0 && norm_out) *norm_out = norm;
  if constexpr (GUARD) { if (!gd->apply) return; }    // (uniform over the grid)
  if (i >= n) return;
  float pi = p[i], mi = m[i], vi = v[i];
  adamw_update(pi, g[i], mi, vi, coef, hp.lr, hp.weight_decay, hp.beta1, hp.beta2, hp.eps, bc1, bc2_sqrt);   // (shared with adamw_groups_kernel: common.h)
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
  if constexpr (EMA) e[i] = ema_update(e[i], pi, ema_w);
}
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ v, long n,
                                                     fv_adamw_hparams hp, float bc1, float bc2_sqrt,
                                                     const float* __restrict__ sumsq, float* __restrict__ norm_out,
                                                     float* __restrict__ e, float ema_w) {
  adamw_body<EMA, false>(p, g, m, v, n, hp, bc1, bc2_sqrt, sumsq, norm_out, e, ema_w, nullptr);
}
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_guard_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, long n,
                                                           fv_adamw_hparams hp, float bc1, float bc2_sqrt,
                                                           const float* __restrict__ sumsq, float* __restrict__ norm_out,
                                                           float* __restrict__ e, float ema_w, const GuardWords* __restrict__ gd) {
  adamw_body<EMA, true>(p, g, m, v, n, hp, bc1, bc2_sqrt, sumsq, norm_out, e, ema_w, gd);
}

// y += x (x != null) or y *= *scale (x == null): gradient accumulation over micro-batches / an upstream loss gradient
__global__ __launch_bounds__(256) void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, long n4,
                                                    const float* __restrict__ scale) {
  const float sc = scale ? *scale : 1.0f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 a = reinterpret_cast<float4*>(y)[i];
    if (x) {
      const float4 b = reinterpret_cast<const float4*>(x)[i];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    } else {
      a.x *= sc; a.y *= sc; a.z *= sc; a.w *= sc;
    }
    reinterpret_cast<float4*>(y)[i] = a;
  }
}

// ---- the step over parameter groups ----
__device__ __forceinline__ float block_sum_256(float s, float* red) {   // every thread returns the block's sum
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[segment] <- sum of squares of the segment's gradient (frozen segments: not read, partial stays 0 as the table's creation left it)
__global__ __launch_bounds__(256) void sumsq_segments_kernel(const float* __restrict__ g, const AdamwSeg* __restrict__ segs, const AdamwGroupDev* __restrict__ groups,
                                                              float* __restrict__ partial) {
  __shared__ float red[4];
  const AdamwSeg sg = segs[blockIdx.x];
  if (groups[sg.group].frozen) return;    // (uniform over the block)
  const float4* g4 = reinterpret_cast<const float4*>(g + sg.begin);
  const int n4 = sg.len >> 2;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 x = g4[i];
    s0 += x.x * x.x; s1 += x.y * x.y; s2 += x.z * x.z; s3 += x.w * x.w;
  }
  const float s = block_sum_256((s0 + s1) + (s2 + s3), red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// phase 0 (one block per group): group_sum[g] <- its segments' partials, thread t taking segments t, t + 256, ... in rising order; 0 for a frozen group.
// phase 1 (one block):           group_sum[n_groups] <- the non-frozen groups' sums, thread t taking groups t, t + 256, ... in rising order.
__global__ __launch_bounds__(256) void sumsq_groups_fold_kernel(const AdamwGroupDev* __restrict__ groups, int n_groups, const float* __restrict__ partial,
                                                                 float* __restrict__ group_sum, int phase) {
  __shared__ float red[4];
  float s = 0.f;
  if (phase == 0) {
    const AdamwGroupDev gr = groups[blockIdx.x];
    if (!gr.frozen)
      for (int i = threadIdx.x; i < gr.seg_count; i += 256) s += partial[gr.seg_begin + i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) group_sum[blockIdx.x] = gr.frozen ? 0.f : s;
  } else {
    for (int i = threadIdx.x; i < n_groups; i += 256)
      if (!groups[i].frozen) s += group_sum[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) group_sum[n_groups] = s;
  }
}

// EMA instance (fv_adamw_clip_step_ema): e, read and written with the same 16-byte accesses, <- ema_update(e, p_new, ema_w) per lane: 4 + 36 bytes per element
// with the norm pass.  A frozen segment's block has left before it touches e.  The plain instance never looks at e / ema_w: it is the kernel as it was.
template <bool EMA, bool GUARD>
__device__ __forceinline__ void adamw_groups_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                  const fv_adamw_hparams& hp, float bc1, float bc2_sqrt, const AdamwSeg* __restrict__ segs,
                                                  const AdamwGroupDev* __restrict__ groups, const float* __restrict__ group_sum, int n_groups,
                                                  float* __restrict__ norm_out, float* __restrict__ group_norms_out, float* __restrict__ e, float ema_w,
                                                  const GuardWords* __restrict__ gd) {
  const AdamwSeg sg = segs[blockIdx.x];
  const AdamwGroupDev gr = groups[sg.group];
  // torch clip_grad_norm_ over the non-frozen elements: coef = clamp(max_norm / (norm + 1e-6), max = 1), as adamw_kernel
  float norm = sqrtf(group_sum[n_groups]) * hp.grad_scale;
  if constexpr (GUARD) norm *= gd->inv_delta;
  float coef = hp.grad_scale;
  if (hp.max_grad_norm > 0.f) coef *= fminf(hp.max_grad_norm / (norm + 1e-6f), 1.0f);
  if constexpr (GUARD) coef *= gd->inv_delta;
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0 && norm_out) *norm_out = norm;
    if (group_norms_out && (int)blockIdx.x == gr.seg_begin) {
      float gn = gr.frozen ? 0.f : sqrtf(group_sum[sg.group]) * hp.grad_scale;
      if constexpr (GUARD) gn *= gd->inv_delta;
      group_norms_out[sg.group] = gn;
    }
  }
  if constexpr (GUARD) { if (!gd->apply) return; }    // (uniform over the grid)
  if (gr.frozen) return;     // p, m, v (and e) keep their bits
  const float lr = hp.lr * gr.lr_scale;
  float4* p4 = reinterpret_cast<float4*>(p + sg.begin);
  float4* m4 = reinterpret_cast<float4*>(m + sg.begin);
  float4* v4 = reinterpret_cast<float4*>(v + sg.begin);
  const float4* g4 = reinterpret_cast<const float4*>(g + sg.begin);
  float4* e4 = EMA ? reinterpret_cast<float4*>(e + sg.begin) : nullptr;
  const int n4 = sg.len >> 2;
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 pi = p4[i], mi = m4[i], vi = v4[i], ei;
    if constexpr (EMA) ei = e4[i];
    const float4 gi = g4[i];
    adamw_update(pi.x, gi.x, mi.x, vi.x, coef, lr, gr.weight_decay, hp.beta1, hp.beta2, hp.eps, bc1, bc2_sqrt);
    adamw_update(pi.y, gi.y, mi.y, vi.y, coef, lr, gr.weight_decay, hp.beta1, hp.beta2, hp.eps, bc1, bc2_sqrt);
    adamw_update(pi.z, gi.z, mi.z, vi.z, coef, lr, gr.weight_decay, hp.beta1, hp.beta2, hp.eps, bc1, bc2_sqrt);
    adamw_update(pi.w, gi.w, mi.w, vi.w, coef, lr, gr.weight_decay, hp.beta1, hp.beta2, hp.eps, bc1, bc2_sqrt);
    p4[i] = pi; m4[i] = mi; v4[i] = vi;
    if constexpr (EMA) {
      ei.x = ema_update(ei.x, pi.x, ema_w); ei.y = ema_update(ei.y, pi.y, ema_w); ei.z = ema_update(ei.z, pi.z, ema_w); ei.w = ema_update(ei.w, pi.w, ema_w);
      e4[i] = ei;
    }
  }
}
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                            fv_adamw_hparams hp, float bc1, float bc2_sqrt, const AdamwSeg* __restrict__ segs,
                                                            const AdamwGroupDev* __restrict__ groups, const float* __restrict__ group_sum, int n_groups,
                                                            float* __restrict__ norm_out, float* __restrict__ group_norms_out, float* __restrict__ e, float ema_w) {
  adamw_groups_body<EMA, false>(p, g, m, v, hp, bc1, bc2_sqrt, segs, groups, group_sum, n_groups, norm_out, group_norms_out, e, ema_w, nullptr);
}
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_groups_guard_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                                  fv_adamw_hparams hp, float bc1, float bc2_sqrt, const AdamwSeg* __restrict__ segs,
                                                                  const AdamwGroupDev* __restrict__ groups, const float* __restrict__ group_sum, int n_groups,
                                                                  float* __restrict__ norm_out, float* __restrict__ group_norms_out, float* __restrict__ e, float ema_w,
                                                                  const GuardWords* __restrict__ gd) {
  adamw_groups_body<EMA, true>(p, g, m, v, hp, bc1, bc2_sqrt, segs, groups, group_sum, n_groups, norm_out, group_norms_out, e, ema_w, gd);
}

// ---- the step guard (fv_step_guard): two one-block kernels over the guard's own 64-byte block
// observe: the handle's fp16 saturation counter against the value seen last; a change sets the sticky flag (the guarded step clears it)
__global__ void step_guard_observe_kernel(GuardWords* __restrict__ w, const unsigned* __restrict__ sat) {
  if (threadIdx.x != 0) return;
  const unsigned c = *sat;
  if (c != w->last_sat) {
    w->last_sat = c;
    if (!(w->flag > 0.f)) w->flag = 1.0f;
  }
}
__global__ void step_guard_report_kernel(const GuardWords* __restrict__ w, float* __restrict__ out) {
  if (threadIdx.x == 0) { out[0] = w->apply ? 0.f : 1.f; out[1] = w->delta; }
}
// decide: the decision of THIS step (apply, 1 / delta) from the sum of squares and the flag, then the state the next forward runs with.  Integers only beyond
// isfinite; tests/step_guard_util.py is the same machine on the host
__global__ void step_guard_decide_kernel(GuardWords* __restrict__ w, const float* __restrict__ sumsq, GuardCfg cfg) {
  if (threadIdx.x != 0) return;
  int dl = w->delta_log2, good = w->good_steps;
  const bool flagged = w->flag > 0.f;
  const bool bad_nonfinite = !isfinite(*sumsq);
  const bool bad_sat = cfg.skip_on_saturation && flagged && dl > cfg.min_log2;
  w->apply = (bad_nonfinite || bad_sat) ? 0 : 1;
  w->inv_delta = ldexpf(1.0f, -dl);
  if (bad_nonfinite || bad_sat) {
    if (bad_nonfinite) w->skipped_nonfinite += 1; else w->skipped_saturated += 1;
    dl = max(cfg.min_log2, dl - cfg.backoff_log2);
    good = 0;
  } else {
    w->applied += 1;
    if (flagged) w->saturated_applied += 1;
    good += 1;
    if (good >= cfg.growth_interval) { dl = min(cfg.max_log2, dl + cfg.growth_log2); good = 0; }
  }
  w->flag = 0.f;
  w->delta_log2 = dl;
  w->good_steps = good;
  w->delta = ldexpf(1.0f, dl);
}

}  // namespace

// the EMA operand of both fused steps: a buffer of its own (the kernels hold p, g, m, v, e as __restrict__) and a weight in [0, 1]
int check_adamw_ema(const char* who, const float* p, const float* g, const float* m, const float* v, const float* ema, float ema_weight, int64_t n) {
  if (!(ema_weight >= 0.f && ema_weight <= 1.f)) return fv_fail(FV_ERR_ARG, "%s: ema_weight %g outside [0, 1]", who, (double)ema_weight);
  const uintptr_t e0 = (uintptr_t)ema, bytes = (uintptr_t)n * sizeof(float);
  const struct { const float* q; const char* name; } others[4] = {{p, "flat_params"}, {g, "flat_grads"}, {m, "m"}, {v, "v"}};
  for (const auto& o : others)
    if (e0 < (uintptr_t)o.q + bytes && (uintptr_t)o.q < e0 + bytes) return fv_fail(FV_ERR_ARG, "%s: ema aliases %s", who, o.name);
  return FV_OK;
}

size_t adamw_scratch_bytes() { return (size_t)(SUMSQ_BLOCKS + 4) * sizeof(float); }

int launch_axpy(float* y, const float* x, int64_t n, const float* scale_dev, hipStream_t s) {
  // the flat head buffers keep every tensor 16-byte aligned and their total a multiple of 4 elements (head_offsets)
  if (n % 4 || ((uintptr_t)y & 15) || ((uintptr_t)x & 15)) return fv_fail(FV_ERR_ARG, "axpy: buffers must be 16-byte aligned, n %% 4 == 0");
  const unsigned nb = cdiv(n / 4, 256);
  hipLaunchKernelGGL(axpy_kernel, dim3(nb < 1024 ? nb : 1024), dim3(256), 0, s, y, x, (long)(n / 4), scale_dev);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

static int adamw_clip_impl(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp,
                           int64_t step, float* norm_scratch, float* grad_norm_out, hipStream_t s, float* ema, float ema_weight, GuardWords* guard, const GuardCfg* cfg) {
  if (!p || !g || !m || !v || !norm_scratch) return fv_fail(FV_ERR_ARG, "adamw: null pointer");
  if (n <= 0 || step < 1) return fv_fail(FV_ERR_ARG, "adamw: n and step must be positive");
  if (ema) { const int rc = check_adamw_ema("adamw", p, g, m, v, ema, ema_weight, n); if (rc != FV_OK) return rc; }
  const unsigned nb = (unsigned)((n + 255) / 256);
  const unsigned nb4 = (unsigned)((n / 4 + 255) / 256 > 0 ? (n / 4 + 255) / 256 : 1);
  const unsigned nsb = nb4 < (unsigned)SUMSQ_BLOCKS ? nb4 : (unsigned)SUMSQ_BLOCKS;
  hipLaunchKernelGGL(sumsq_kernel, dim3(nsb), dim3(256), 0, s, g, (long)n, norm_scratch);
  hipLaunchKernelGGL(sumsq_fold_kernel, dim3(1), dim3(256), 0, s, norm_scratch, (int)nsb);
  const float bc1 = (float)(1.0 - pow((double)hp.beta1, (double)step));
  const float bc2 = (float)sqrt(1.0 - pow((double)hp.beta2, (double)step));
  if (guard) {
    hipLaunchKernelGGL(step_guard_decide_kernel, dim3(1), dim3(64), 0, s, guard, (const float*)norm_scratch, *cfg);
    if (ema && ema_weight != 0.f)
      hipLaunchKernelGGL(adamw_guard_kernel<true>, dim3(nb), dim3(256), 0, s, p, g, m, v, (long)n, hp, bc1, bc2, (const float*)norm_scratch, grad_norm_out, ema, ema_weight,
                         (const GuardWords*)guard);
    else
      hipLaunchKernelGGL(adamw_guard_kernel<false>, dim3(nb), dim3(256), 0, s, p, g, m, v, (long)n, hp, bc1, bc2, (const float*)norm_scratch, grad_norm_out, (float*)nullptr, 0.f,
                         (const GuardWords*)guard);
  } else if (ema && ema_weight != 0.f)   // (weight 0 leaves the average alone: the plain instance, which never reads it)
    hipLaunchKernelGGL(adamw_kernel<true>, dim3(nb), dim3(256), 0, s, p, g, m, v, (long)n, hp, bc1, bc2, (const float*)norm_scratch, grad_norm_out, ema, ema_weight);
  else
    hipLaunchKernelGGL(adamw_kernel<false>, dim3(nb), dim3(256), 0, s, p, g, m, v, (long)n, hp, bc1, bc2, (const float*)norm_scratch, grad_norm_out, (float*)nullptr, 0.f);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
int launch_adamw_clip(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp,
                      int64_t step, float* norm_scratch, float* grad_norm_out, hipStream_t s, float* ema, float ema_weight) {
  return adamw_clip_impl(p, g, m, v, n, hp, step, norm_scratch, grad_norm_out, s, ema, ema_weight, nullptr, nullptr);
}
int launch_adamw_clip_guarded(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp, int64_t step, float* norm_scratch,
                              float* grad_norm_out, hipStream_t s, float* ema, float ema_weight, GuardWords* guard, const GuardCfg& cfg) {
  if (!guard) return fv_fail(FV_ERR_ARG, "adamw: null guard");
  return adamw_clip_impl(p, g, m, v, n, hp, step, norm_scratch, grad_norm_out, s, ema, ema_weight, guard, &cfg);
}
int launch_guard_report(const GuardWords* w, float* out2, hipStream_t s) {
  if (!w || !out2) return fv_fail(FV_ERR_ARG, "step guard report: null pointer");
  hipLaunchKernelGGL(step_guard_report_kernel, dim3(1), dim3(64), 0, s, w, out2);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
int launch_guard_observe(GuardWords* w, const unsigned* sat_counter, hipStream_t s) {
  if (!w || !sat_counter) return fv_fail(FV_ERR_ARG, "step guard observe: null pointer");
  hipLaunchKernelGGL(step_guard_observe_kernel, dim3(1), dim3(64), 0, s, w, sat_counter);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

static int adamw_clip_groups_impl(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp, const AdamwGroupsTable& t,
                                  int64_t step, float* grad_norm_out, float* group_norms_out, hipStream_t s, float* ema, float ema_weight, GuardWords* guard,
                                  const GuardCfg* cfg) {
  if (!p || !g || !m || !v || !t.segs || !t.groups || !t.sums) return fv_fail(FV_ERR_ARG, "adamw groups: null pointer");
  if (step < 1) return fv_fail(FV_ERR_ARG, "adamw groups: step must be positive");
  if (n != t.n) return fv_fail(FV_ERR_ARG, "adamw groups: n = %lld, the table was built for %lld", (long long)n, (long long)t.n);
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) != 0) return fv_fail(FV_ERR_ARG, "adamw groups: buffers must be 16-byte aligned");
  if (t.n_segs <= 0 || t.n_groups <= 0) return fv_fail(FV_ERR_ARG, "adamw groups: empty table");
  if (ema) {
    if (((uintptr_t)ema & 15) != 0) return fv_fail(FV_ERR_ARG, "adamw groups: ema must be 16-byte aligned");
    const int rc = check_adamw_ema("adamw groups", p, g, m, v, ema, ema_weight, n);
    if (rc != FV_OK) return rc;
  }
  float* group_sum = t.sums + t.n_segs;
  hipLaunchKernelGGL(sumsq_segments_kernel, dim3(t.n_segs), dim3(256), 0, s, g, t.segs, t.groups, t.sums);
  hipLaunchKernelGGL(sumsq_groups_fold_kernel, dim3(t.n_groups), dim3(256), 0, s, t.groups, t.n_groups, (const float*)t.sums, group_sum, 0);
  hipLaunchKernelGGL(sumsq_groups_fold_kernel, dim3(1), dim3(256), 0, s, t.groups, t.n_groups, (const float*)t.sums, group_sum, 1);
  const float bc1 = (float)(1.0 - pow((double)hp.beta1, (double)step));
  const float bc2 = (float)sqrt(1.0 - pow((double)hp.beta2, (double)step));
  if (guard) {
    hipLaunchKernelGGL(step_guard_decide_kernel, dim3(1), dim3(64), 0, s, guard, (const float*)(group_sum + t.n_groups), *cfg);
    if (ema && ema_weight != 0.f)
      hipLaunchKernelGGL(adamw_groups_guard_kernel<true>, dim3(t.n_segs), dim3(256), 0, s, p, g, m, v, hp, bc1, bc2, t.segs, t.groups, (const float*)group_sum, t.n_groups,
                         grad_norm_out, group_norms_out, ema, ema_weight, (const GuardWords*)guard);
    else
      hipLaunchKernelGGL(adamw_groups_guard_kernel<false>, dim3(t.n_segs), dim3(256), 0, s, p, g, m, v, hp, bc1, bc2, t.segs, t.groups, (const float*)group_sum, t.n_groups,
                         grad_norm_out, group_norms_out, (float*)nullptr, 0.f, (const GuardWords*)guard);
  } else if (ema && ema_weight != 0.f)   // (weight 0 leaves the average alone: the plain instance, which never reads it)
    hipLaunchKernelGGL(adamw_groups_kernel<true>, dim3(t.n_segs), dim3(256), 0, s, p, g, m, v, hp, bc1, bc2, t.segs, t.groups, (const float*)group_sum, t.n_groups,
                       grad_norm_out, group_norms_out, ema, ema_weight);
  else
    hipLaunchKernelGGL(adamw_groups_kernel<false>, dim3(t.n_segs), dim3(256), 0, s, p, g, m, v, hp, bc1, bc2, t.segs, t.groups, (const float*)group_sum, t.n_groups,
                       grad_norm_out, group_norms_out, (float*)nullptr, 0.f);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
int launch_adamw_clip_groups(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp, const AdamwGroupsTable& t,
                             int64_t step, float* grad_norm_out, float* group_norms_out, hipStream_t s, float* ema, float ema_weight) {
  return adamw_clip_groups_impl(p, g, m, v, n, hp, t, step, grad_norm_out, group_norms_out, s, ema, ema_weight, nullptr, nullptr);
}
int launch_adamw_clip_groups_guarded(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp, const AdamwGroupsTable& t, int64_t step,
                                     float* grad_norm_out, float* group_norms_out, hipStream_t s, float* ema, float ema_weight, GuardWords* guard, const GuardCfg& cfg) {
  if (!guard) return fv_fail(FV_ERR_ARG, "adamw groups: null guard");
  return adamw_clip_groups_impl(p, g, m, v, n, hp, t, step, grad_norm_out, group_norms_out, s, ema, ema_weight, guard, &cfg);
}

}  // namespace fv
