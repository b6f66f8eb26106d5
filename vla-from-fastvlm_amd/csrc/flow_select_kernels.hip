// flow_select_kernels.hip -- the choice among the S candidates of a multi-sample call (fv_head_flow_sample_multi), all fp32, every sum in a fixed order:
//   flow_select_kernel    one block per observation: pairwise squared distances, the score of every candidate, the choice, and every output of the call
// The candidates are the sampler's normalised rows, sample-major (row s B + b); nothing here multiplies the chosen one except the single folded
// un-normalisation that every sampler applies.
#include "kernels.h"

namespace fv {
namespace {

constexpr int SEL_MAX = FV_FLOW_SAMPLES_MAX;

// 256 threads = 4 waves, block b = observation b.  No atomics; two runs give the same bits.
//   distances  the unordered pairs (i < j) are numbered p = 0, 1, .. in the order (0,1), (0,2), .., (1,2), ..; wave w takes the pairs with p % 4 == w.  Lane l
//              adds (x_i[e] - x_j[e])^2 over e = l, l + 64, .. in ascending e, one wave_sum per pair; D[i][j] = D[j][i] in LDS, each pair computed once
//   finite     a candidate with a NaN or +-inf element is set aside: its score is +inf whatever the mode, and the MEDOID sums of the others skip it
//   MEDOID     score[s] = D[s][0] + D[s][1] + .. in ascending s' (D[s][s] = 0)
//   COHERENT   score[s] = sum_{k < K - shift} w[k] sum_a (x_s[k][a] - prev[b][k + shift][a])^2: wave w takes candidates w, w + 4, ..; lane l adds
//              w[e / A] (x_s[e] - prev[b][e + shift A])^2 over e = l, l + 64, .. < (K - shift) A, one wave_sum per candidate.  A weight of 0 SELECTS the
//              term away, and prev beyond the overlap is never read.  A row whose row_mask is 0 takes the MEDOID score
//   FIRST      the MEDOID scores are reported, candidate 0 is chosen
//   choice     the smallest score in ascending s, a non-finite score counting as +inf (and reported as +inf): ties, and a row without a finite score, go to
//              the lowest index
//   outputs    chunk_out = a copy of the chosen row; actions = flow_fma's x std + mean (or x); spread = the population standard deviation over s per
//              element, two passes in ascending s; candidates_out = a copy of the S rows.  (With S == 1 cand may BE chunk_out: every element is read and
//              written back by the one thread that owns it)
__global__ __launch_bounds__(256) void flow_select_kernel(const float* cand, int B, int S, int da, FlowSelect sel, const float* __restrict__ post_scale,
                                                           const float* __restrict__ post_shift) {
  __shared__ float D[SEL_MAX][SEL_MAX + 1];
  __shared__ float score[SEL_MAX];
  __shared__ int pick, bad[SEL_MAX];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, tid = threadIdx.x;
  auto row = [&](int s) { return cand + ((size_t)s * B + b) * da; };
  const bool coherent = sel.mode == FV_FLOW_SELECT_COHERENT && (!sel.row_mask || sel.row_mask[b] != 0);
  for (int s = wv; s < S; s += 4) {   // 0 x is 0 for a finite x and NaN for NaN and +-inf: the sum says whether the whole row is finite
    const float* xs = row(s);
    float acc = 0.f;
    for (int e = lane; e < da; e += 64) acc += xs[e] * 0.f;
    acc = wave_sum(acc);
    if (lane == 0) bad[s] = acc == 0.f ? 0 : 1;
  }
  if (!coherent) {
    if (tid < S) D[tid][tid] = 0.f;
    int p = 0;
    for (int i = 0; i < S; ++i)
      for (int j = i + 1; j < S; ++j, ++p) {
        if ((p & 3) != wv) continue;
        const float *xi = row(i), *xj = row(j);
        float acc = 0.f;
        for (int e = lane; e < da; e += 64) { const float df = xi[e] - xj[e]; acc += df * df; }
        acc = wave_sum(acc);
        if (lane == 0) D[i][j] = D[j][i] = acc;
      }
    __syncthreads();
    if (tid < S) {
      float sc = 0.f;
      for (int s2 = 0; s2 < S; ++s2) sc += bad[s2] ? 0.f : D[tid][s2];
      score[tid] = sc;
    }
  } else {
    const int A = da / sel.chunk, live = (sel.chunk - sel.shift) * A;
    const float* y = sel.prev + (size_t)b * da + (size_t)sel.shift * A;   // (e + shift A < K A = da)
    for (int s = wv; s < S; s += 4) {
      const float* xs = row(s);
      float acc = 0.f;
      for (int e = lane; e < live; e += 64) {
        const float w = sel.step_w[e / A];
        if (w != 0.f) { const float df = xs[e] - y[e]; acc += w * (df * df); }
      }
      acc = wave_sum(acc);
      if (lane == 0) score[s] = acc;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    float best = __builtin_inff();
    for (int s = 0; s < S; ++s) {
      const float v = !bad[s] && __builtin_isfinite(score[s]) ? score[s] : __builtin_inff();
      if (sel.scores_out) sel.scores_out[(size_t)b * S + s] = v;
      if (v < best) { best = v; c = s; }
    }
    if (sel.mode == FV_FLOW_SELECT_FIRST) c = 0;
    if (sel.choice_out) sel.choice_out[b] = c;
    pick = c;
  }
  __syncthreads();
  const float* xc = row(pick);
  for (int e = tid; e < da; e += 256) {
    const float x = xc[e];
    sel.chunk_out[(size_t)b * da + e] = x;
    sel.actions[(size_t)b * da + e] = post_scale ? __builtin_fmaf(x, post_scale[e], post_shift[e]) : x;
    if (sel.spread_out) {
      float sum = 0.f;
      for (int s = 0; s < S; ++s) sum += row(s)[e];
      const float mean = sum / (float)S;
      float q = 0.f;
      for (int s = 0; s < S; ++s) { const float df = row(s)[e] - mean; q += df * df; }
      sel.spread_out[(size_t)b * da + e] = sqrtf(q / (float)S);
    }
    if (sel.candidates_out)
      for (int s = 0; s < S; ++s) sel.candidates_out[((size_t)s * B + b) * da + e] = row(s)[e];
  }
}

}  // namespace

int flow_select_check(const FlowSelect& sel, int S, int da) {
  if (S < 1 || S > SEL_MAX) return fv_fail(FV_ERR_ARG, "flow_select: S = %d outside 1 .. %d", S, SEL_MAX);
  if (sel.mode != FV_FLOW_SELECT_FIRST && sel.mode != FV_FLOW_SELECT_MEDOID && sel.mode != FV_FLOW_SELECT_COHERENT)
    return fv_fail(FV_ERR_ARG, "flow_select: unknown select %d (0 first, 1 medoid, 2 coherent)", sel.mode);
  if (!sel.actions || !sel.chunk_out) return fv_fail(FV_ERR_ARG, "flow_select: null pointer");
  if (sel.mode == FV_FLOW_SELECT_COHERENT) {
    if (!sel.step_w || sel.chunk < 1 || da % sel.chunk) return fv_fail(FV_ERR_STATE, "flow_select: coherent selection has no step weights (fv_head_set_flow_samples)");
    if (!sel.prev) return fv_fail(FV_ERR_ARG, "flow_select: coherent selection needs prev");
    if (sel.shift < 0 || sel.shift > sel.chunk) return fv_fail(FV_ERR_ARG, "flow_select: shift = %d outside 0 .. chunk = %d", sel.shift, sel.chunk);
  }
  return FV_OK;
}

int launch_flow_select(const float* cand, int B, int S, int da, const FlowSelect& sel, const float* post_scale, const float* post_shift, hipStream_t s) {
  if (!cand || B < 1 || da < 1) return fv_fail(FV_ERR_ARG, "flow_select: bad argument");
  if (!post_scale != !post_shift) return fv_fail(FV_ERR_ARG, "flow_select: give both action statistics or neither");
  if (const int rc = flow_select_check(sel, S, da)) return rc;
  hipLaunchKernelGGL(flow_select_kernel, dim3(B), dim3(256), 0, s, cand, B, S, da, sel, post_scale, post_shift);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

}  // namespace fv
