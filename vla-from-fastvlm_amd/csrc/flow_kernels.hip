// flow_kernels.hip -- the flow-matching form of the action expert (fv_head_set_flow), all fp32, every sum in a fixed order:
//   flow_prepare_kernel                    training: x_t and phi(t) into their columns of the head's cat, u = eps - a as the loss target; the head itself
//                                          (head_kernels.hip) then runs forward and backward as it does for regression
//   flow_time / flow_beta_inv              the training time as an inverse CDF (fv_head_set_flow_time): Beta, range and strata from the row's one uniform, in the
//                                          <FlowTimeArgs> instances of flow_prepare_kernel -- a handle without the setting launches the plain ones
//   flow_cond / _init / _step_a / _b / _c  the sampler (fv_head_flow_sample): conditioning once, three launches per network evaluation
//   <PREFIX> instances                     action-prefix conditioning (fv_head_set_flow_prefix): what the noising step, the conditioning, the start and step C
//                                          add for it sits under `if constexpr (PREFIX)` in the one body each of them has
//   flow_guide_* / flow_vjp_t_kernel       guided sampling (fv_head_set_flow_guidance; real-time chunking): the step's forward with z3 and v kept, J^T omega
//                                          through three transposed products and a LayerNorm backward, and the update
//   flow_cond_broadcast_kernel             several samples per observation (fv_head_flow_sample_multi): the start runs on a (B, S) grid, the conditioning on B
//                                          rows and is copied, the steps run unchanged on S B rows; the choice among them is flow_select_kernels.hip's
//   flow_rk_stage                          the x update of every solver (fv_head_set_flow_solver), in step C and in the guided update: an explicit
//                                          Runge-Kutta stage, Euler being the scheme with one (FLOW_TABLEAUX); flow_integrate is the one loop over them
// The state branch of every sampler is head_kernels.hip's (launch_head_state_branch); the draws come from common.h philox under this file's key.
#include "kernels.h"

#include <algorithm>

namespace fv {
namespace {

// ---- flow-matching head (fv_head_set_flow): x_t = t eps + (1 - t) a, u = eps - a; sampling runs x <- x + dt v from t = 1 to t = 0 ----
// The draws are Philox4x32-10 under a key of their own (the dropout stream of the same (seed, offset) is another stream); the counter is
// (group, row, offset): group 0 is the row's t, group 1 + i / 4 the normals of elements 4 (i / 4) .. + 3 -- a function of (row, element) only, so row b draws
// the same values whatever B and the launch geometry are.
constexpr uint32_t FLOW_KEY_LO = 0x464C4F57u, FLOW_KEY_HI = 0x4D415443u;
constexpr float FLOW_TWO_PI = 6.28318530717958647692f, FLOW_U24 = 1.0f / 16777216.0f;
__device__ __forceinline__ uint4 flow_philox(uint32_t group, uint32_t row, uint64_t seed, uint64_t offset) {
  return philox(make_uint4(group, row, (uint32_t)offset, (uint32_t)(offset >> 32)), make_uint2((uint32_t)seed ^ FLOW_KEY_LO, (uint32_t)(seed >> 32) ^ FLOW_KEY_HI));
}
// Box-Muller on two 24-bit uniforms, u1 in (0, 1] and u2 in [0, 1): (r cos, r sin) with r = sqrt(-2 log u1).  sinf / cosf / logf, not the fast intrinsics
__device__ __forceinline__ float2 flow_box_muller(uint32_t a, uint32_t b) {
  const float u1 = (float)((a >> 8) + 1u) * FLOW_U24, u2 = (float)(b >> 8) * FLOW_U24;
  const float r = sqrtf(-2.0f * logf(u1)), th = FLOW_TWO_PI * u2;
  return make_float2(r * cosf(th), r * sinf(th));
}
__device__ __forceinline__ void flow_normals4(uint32_t group, uint32_t row, uint64_t seed, uint64_t offset, float (&n)[4]) {
  const uint4 r = flow_philox(group, row, seed, offset);
  const float2 p = flow_box_muller(r.x, r.y), q = flow_box_muller(r.z, r.w);
  n[0] = p.x; n[1] = p.y; n[2] = q.x; n[3] = q.y;
}
// phi(t) = [ sin(freq_j t) | cos(freq_j t) ], j < te / 2; the argument is ONE fp32 product (it reaches ~1600 rad: sinf / cosf reduce it properly)
__device__ __forceinline__ void flow_phi(float* __restrict__ dst, const float* __restrict__ freq, int half, float t, int i) {
  const float arg = freq[i] * t;
  dst[i] = sinf(arg);
  dst[half + i] = cosf(arg);
}

// ---- the training time as an inverse CDF (fv_head_set_flow_time): tau = F^-1(u) in double from the row's one uniform.  Every thread of the block runs the
// same arithmetic on the same u, so the control flow below is uniform over the block: no barrier, no hand-over, no atomics; every loop has a cap.
// The continued fraction of I_x(a, b) (modified Lentz), for x <= (a + 1) / (a + b + 2) where it converges in O(sqrt(max(a, b))) terms:
//     I_x(a, b) = x^a (1 - x)^b / (a B(a, b)) * cf
constexpr int FLOW_BETA_CF_MAX = 300, FLOW_BETA_NEWTON_MAX = 64;
__device__ double flow_beta_cf(double a, double b, double x) {
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0, tiny = 1e-300;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= FLOW_BETA_CF_MAX; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 3e-16) break;
  }
  return h;
}
// x in (0, xhi] with I_x(a, b) = p, for 0 < p <= I_xhi(a, b) and xhi <= (a + 1) / (a + b + 2).  Newton on g(y) = log I_{exp y} - log p in y = log x, where g is
// close to a line of slope a for small x and g'(y) = a / ((1 - x) cf): the RELATIVE error of x is what converges, down to x = 1e-300.  lab = log(a B(a, b)).
// Safeguard: the iterate stays inside the bracket the signs of g have drawn so far, by bisection where Newton would leave it.  It stops once a NEWTON step is
// below 1e-9 (the error behind a quadratically convergent step of that size is far below 2^-40) or the bracket is narrower than 1e-14, at the cap otherwise
__device__ double flow_beta_inv_lower(double a, double b, double lab, double p, double xhi) {
  const double lp = log(p);
  double ylo = -700.0, yhi = log(xhi);
  double y = fmin(fmax((lp + lab) / a, ylo), yhi);
  bool top = false;   // the upper end itself has been evaluated
  for (int it = 0; it < FLOW_BETA_NEWTON_MAX; ++it) {
    const double x = exp(y), cf = flow_beta_cf(a, b, x);
    const double g = a * y + b * log1p(-x) - lab + log(cf) - lp;
    if (g == 0.0) break;
    top = top || y == yhi;
    if (g > 0.0) yhi = y; else ylo = y;
    double yn = y - g * (1.0 - x) * cf / a;
    bool newton = true;
    if (yn > yhi && !top) yn = yhi;   // (a root at the end of the range: look at the end before halving towards it)
    else if (!(yn >= ylo && yn <= yhi)) { yn = 0.5 * (ylo + yhi); newton = false; }
    const double dy = yn - y;
    y = yn;
    if ((newton && fabs(dy) < 1e-9) || yhi - ylo < 1e-14) break;   // (a halving step says nothing about the error: only the bracket's width ends those)
  }
  return exp(y);
}
// tau = I^-1_u(a, b).  The closed forms of a = 1 and b = 1 (pi0's Beta(1.5, 1) is u^(1 / 1.5)) keep the relative accuracy of exp / log / expm1 / log1p in double.
// Otherwise the tail is chosen at xs = (a + 1) / (a + b + 2), where both continued fractions converge: the lower one solves for x, the upper one for 1 - x in
// Beta(b, a) at 1 - u (exact in double for u >= 1 / 2), so a tau near 0 keeps its relative and a tau near 1 its absolute accuracy
__device__ double flow_beta_inv(double a, double b, double lbeta, double u) {
  if (u <= 0.0) return 0.0;
  if (a == 1.0 && b == 1.0) return u;
  if (b == 1.0) return exp(log(u) / a);
  if (a == 1.0) return -expm1(log1p(-u) / b);
  const double xs = (a + 1.0) / (a + b + 2.0), la = log(a) + lbeta, lb = log(b) + lbeta;
  const double ps = exp(a * log(xs) + b * log1p(-xs) - la) * flow_beta_cf(a, b, xs);
  if (u <= ps) return flow_beta_inv_lower(a, b, la, u, xs);
  return 1.0 - flow_beta_inv_lower(b, a, lb, 1.0 - u, 1.0 - xs);
}
// the row's time from k, the 24-bit integer behind the uniform t (s of S: the stratum; S == 1: none).  t = t_lo + (t_hi - t_lo) tau in double, rounded once.
// bm: the fp32 logit-normal tau of the unstratified form, fv_head_set_flow's expression with its bits
struct FlowTimeArgs { int dist, strat; double a, b, lbeta, t_lo, t_span; };
__device__ float flow_time(const FlowTimeArgs& tm, uint32_t k, uint32_t s, uint32_t S, float bm) {
  double u = (double)k * (1.0 / 16777216.0);
  if (tm.strat) u = ((double)s + u) / (double)S;
  double tau;
  if (tm.dist == 2) tau = flow_beta_inv(tm.a, tm.b, tm.lbeta, u);
  else if (tm.dist == 0) tau = u;
  else if (!tm.strat) tau = (double)bm;
  else tau = u <= 0.0 ? 0.0 : 1.0 / (1.0 + exp(-(tm.a + tm.b * normcdfinv(u))));
  return (float)(tm.t_lo + tm.t_span * tau);
}

// block = one head row, grid (B, S): head row r = s B + b is draw s of observation b (fv_head_set_flow_draws; S == 1: the rows as ever).  It reads targets[b]
// and draws what row b draws at offset + (s << 56) -- the key, the counter (group, b, offset) and the Box-Muller as they are, so row b's draws depend
// neither on B nor on S, and draw 0 is the single draw.  Explicit noise (S B, da) / tin (S B) are read at r.
// cat: the row-major (S B, cw) matrix inside `saved`; columns [xo, xo + da) <- x_t, [xo + da, xo + da + te) <- phi(t); u_out (S B, da) <- eps - a.
// x_t is formed in double and rounded once: t eps and (1 - t) a cancel for some rows, and the fp32 form then loses bits the loss target does not.
// PREFIX (fv_head_set_flow_prefix): the row's delay d is delays[row] clamped to 0 .. pd, or the smallest j with (z >> 8) < thr[j], z the third word of the
// group-0 block whose x and y yield t (an integer compare; no new stream, no new counter: t and eps are the plain head's bits).  The first d steps of x_t are
// COPIES of targets, m = [k < d] goes behind phi(t) as exact 0.0 / 1.0 and as bytes into pmask; u is written everywhere as ever
// TM (fv_head_set_flow_time): empty, or one FlowTimeArgs behind the plain arguments -- the drawn t then goes through flow_time.  Instances of their own with
// an argument of their own: a handle without the setting launches the kernels, with the arguments, it always did
struct FlowPrefixArgs { const int32_t* delays; const uint32_t* thr; uint8_t* pmask; int pk, pd; };
template <bool PREFIX, class... TM>
__global__ __launch_bounds__(256) void flow_prepare_kernel(const float* __restrict__ targets, const float* __restrict__ noise, const float* __restrict__ tin,
                                                            float* __restrict__ cat, int cw, int xo, float* __restrict__ u_out, int da, int te,
                                                            const float* __restrict__ freq, int time_dist, float dist_a, float dist_b, uint64_t seed,
                                                            uint64_t offset, FlowPrefixArgs px, TM... tma) {
  static_assert(sizeof...(TM) <= 1, "at most one FlowTimeArgs");
  const int obs = blockIdx.x, row = blockIdx.y * gridDim.x + obs;
  offset += (uint64_t)blockIdx.y << 56;
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (PREFIX || !tin) r = flow_philox(0u, (uint32_t)obs, seed, offset);   // (PREFIX: a drawn delay needs the block with t given, too)
  float t;
  if (tin) t = tin[row];
  else if constexpr (sizeof...(TM) != 0) {
    const FlowTimeArgs& tm = (tma, ...);
    const float bm = tm.dist == 1 && !tm.strat ? 1.0f / (1.0f + expf(-(dist_a + dist_b * flow_box_muller(r.x, r.y).x))) : 0.f;
    t = flow_time(tm, r.x >> 8, blockIdx.y, gridDim.y, bm);
  }
  else if (time_dist == 0) t = (float)(r.x >> 8) * FLOW_U24;
  else t = 1.0f / (1.0f + expf(-(dist_a + dist_b * flow_box_muller(r.x, r.y).x)));
  float* xr = cat + (size_t)row * cw + xo;
  int pin = 0;   // elements [0, pin) of the row are the conditioned steps
  if constexpr (PREFIX) {
    int dl = 0;
    if (px.delays) {
      dl = min(max(px.delays[row], 0), px.pd);
    } else {
      const uint32_t z24 = r.z >> 8;
      while (dl < px.pd && z24 >= px.thr[dl]) ++dl;
    }
    pin = dl * (da / px.pk);
    for (int k = threadIdx.x; k < px.pk; k += 256) {
      xr[da + te + k] = k < dl ? 1.0f : 0.0f;
      px.pmask[(size_t)row * px.pk + k] = k < dl ? 1 : 0;
    }
  }
  const double td = (double)t, omt = 1.0 - td;
  for (int g = threadIdx.x; g * 4 < da; g += 256) {
    float n[4] = {0.f, 0.f, 0.f, 0.f};
    if (!noise) flow_normals4(1u + (uint32_t)g, (uint32_t)obs, seed, offset, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = g * 4 + j;
      if (i >= da) break;
      const float e = noise ? noise[(size_t)row * da + i] : n[j], a = targets[(size_t)obs * da + i];
      xr[i] = PREFIX && i < pin ? a : (float)(td * (double)e + omt * (double)a);
      u_out[(size_t)row * da + i] = e - a;
    }
  }
  for (int i = threadIdx.x; i < te / 2; i += 256) flow_phi(xr + da, freq, te / 2, t, i);
}

// ---- the prefix sampler (fv_head_flow_sample_prefix; training-time action conditioning): the PREFIX instances of the start, the conditioning and step C.
// Row b's first p_b = min(delays[b], pd, chunk - shift) steps are PINNED to prev[b][k + shift]: written once by the start kernel, left alone by every step, so
// they leave as the bits they came in with.  The clamp runs inside the kernels (no host synchronisation); a pinned element is SELECTED, whatever prev holds
// elsewhere (NaN, +-inf) is never read.  The plain instances get an empty FlowPinned and read none of it
struct FlowPinned { const float* prev; const int32_t* delays; int pd, chunk, shift; };
__device__ __forceinline__ int flow_pinned_steps(const FlowPinned& p, int b) { return min(min(max(p.delays[b], 0), p.pd), p.chunk - p.shift); }

// the sampler's start: xphi (S B, da + te) <- [ noise or the draws of (seed, offset); PREFIX: prev on the pinned elements | phi(t0) ]
// grid (B, S): block (b, s) writes head row r = s B + b, candidate s of observation b (fv_head_set_flow_samples; S == 1: blockIdx.y == 0, the rows and the
// arithmetic as ever).  It draws what row b draws at offset + (s << 56) -- the counter is (group, b, offset) --, so candidate s is the single-sample call at
// that offset and candidate 0 is today's sample.  Explicit noise (S B, da) is read at r.  PREFIX: prev / delays are observation b's; delays_rows (S B) or null
// takes a copy of the row's delay, which step C then reads per head row
template <bool PREFIX>
__global__ __launch_bounds__(256) void flow_init_kernel(const float* __restrict__ noise, float* __restrict__ xphi, int da, int te, const float* __restrict__ freq,
                                                         float t0, uint64_t seed, uint64_t offset, FlowPinned p, int32_t* __restrict__ delays_rows) {
  const int obs = blockIdx.x, row = blockIdx.y * gridDim.x + obs;
  offset += (uint64_t)blockIdx.y << 56;
  int A = 0, pin = 0;
  if constexpr (PREFIX) {
    A = da / p.chunk;
    pin = flow_pinned_steps(p, obs) * A;
    if (delays_rows && threadIdx.x == 0) delays_rows[row] = p.delays[obs];
  }
  float* xr = xphi + (size_t)row * (da + te);
  for (int g = threadIdx.x; g * 4 < da; g += 256) {
    float n[4] = {0.f, 0.f, 0.f, 0.f};
    if (!noise) flow_normals4(1u + (uint32_t)g, (uint32_t)obs, seed, offset, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = g * 4 + j;
      if (i >= da) break;
      if (PREFIX && i < pin) xr[i] = p.prev[(size_t)obs * da + i + (size_t)p.shift * A];   // (i + shift A < (p_b + shift) A <= da)
      else xr[i] = noise ? noise[(size_t)row * da + i] : n[j];
    }
  }
  for (int i = threadIdx.x; i < te / 2; i += 256) flow_phi(xr + da, freq, te / 2, t0, i);
}
// c (B, n) -> the rows of candidates 1 .. S - 1 (grid.y = S - 1): the conditioning depends on the observation only, so it is computed on B rows and copied
__global__ __launch_bounds__(256) void flow_cond_broadcast_kernel(float* __restrict__ c, int B, int n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * n) return;
  c[(size_t)(1 + blockIdx.y) * B * n + i] = c[i];
}

// The sampler's products keep linear_fwd_kernel's layout: one wave per output column n, 8 batch rows per pass, coalesced weight reads, a wave_sum per row
// (a fixed order: two runs give the same bits).  wr: row n of the weight, or a column range of it.
__device__ __forceinline__ void flow_dot8(const float* __restrict__ x, int ldx, const float* __restrict__ wr, int K, int b0, int B, int lane, float (&acc)[8]) {
  for (int k = lane; k < K; k += 64) {
    const float wv = wr[k];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += x[(size_t)min(b0 + j, B - 1) * ldx + k] * wv;
  }
}
// once per call: c[b][n] = b4[n] + W4[n][0 : feat] . pooled[b] + W4[n][feat : feat + hid] . s[b]  (the part of fusion.0 that does not depend on t)
// PREFIX: the mask block as well, c[b][n] += sum_{k < p_b} W4[n][mo + k], which does not change over the steps.  The mask's columns join the wave's partial
// sums behind the state branch's (lane k % 64 owns column k), one wave_sum per row as ever: a fixed order
template <bool PREFIX>
__global__ __launch_bounds__(256) void flow_cond_kernel(const float* __restrict__ pooled, int feat, const float* __restrict__ sb, int hid, const float* __restrict__ W,
                                                         int ldw, const float* __restrict__ bias, float* __restrict__ c, int B, int N, int mo, FlowPinned p) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), b0 = blockIdx.y * 8;
  if (n >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  flow_dot8(pooled, feat, W + (size_t)n * ldw, feat, b0, B, lane, acc);
  flow_dot8(sb, hid, W + (size_t)n * ldw + feat, hid, b0, B, lane, acc);
  if constexpr (PREFIX) {
    int pin[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) pin[j] = flow_pinned_steps(p, min(b0 + j, B - 1));
    for (int k = lane; k < p.pd; k += 64) {   // (p_b <= pd: the columns behind it are never read)
      const float wv = W[(size_t)n * ldw + mo + k];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += k < pin[j] ? wv : 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0)
    for (int j = 0; j < 8 && b0 + j < B; ++j) c[(size_t)(b0 + j) * N + n] = acc[j] + bias[n];
}
// step kernel A: z2[b][n] = c[b][n] + W4[n][xo : xo + xw] . [x | phi(t_i)][b]
__global__ __launch_bounds__(256) void flow_step_a_kernel(const float* __restrict__ xphi, int xw, const float* __restrict__ W, int ldw, int xo,
                                                           const float* __restrict__ c, float* __restrict__ z2, int B, int N) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), b0 = blockIdx.y * 8;
  if (n >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  flow_dot8(xphi, xw, W + (size_t)n * ldw + xo, xw, b0, B, lane, acc);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0)
    for (int j = 0; j < 8 && b0 + j < B; ++j) z2[(size_t)(b0 + j) * N + n] = c[(size_t)(b0 + j) * N + n] + acc[j];
}
// step kernel B: a3[b][n] = silu(b8[n] + W8[n] . silu(LN(z2[b]))).  Every block recomputes the statistics of its 8 rows (wave w: rows 2w, 2w + 1; ln_fwd_kernel's
// two passes and order) and applies LayerNorm and SiLU while it loads: no normalised copy travels through memory and no block waits for another
// STASH (the guided step): the pre-activation z3 = b8 + W8 . silu(LN(z2)) is kept as well, for silu' in the backward chain; nothing else differs
template <bool STASH>
__global__ __launch_bounds__(256) void flow_step_b_kernel(const float* __restrict__ z2, const float* __restrict__ lw, const float* __restrict__ lb,
                                                           const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ a3,
                                                           float* __restrict__ z3, int B, int N) {
  __shared__ float st[2][8];   // mean, rstd
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = blockIdx.x * 4 + wv, b0 = blockIdx.y * 8;
  for (int r = 2 * wv; r < 2 * wv + 2; ++r) {
    const float* zr = z2 + (size_t)min(b0 + r, B - 1) * N;
    float s = 0.f;
    for (int i = lane; i < N; i += 64) s += zr[i];
    const float mean = wave_sum(s) / (float)N;
    float q = 0.f;
    for (int i = lane; i < N; i += 64) { const float d = zr[i] - mean; q += d * d; }
    const float rs = rsqrtf(wave_sum(q) / (float)N + LN_EPS);
    if (lane == 0) { st[0][r] = mean; st[1][r] = rs; }
  }
  __syncthreads();
  if (n >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const float* wr = W + (size_t)n * N;
  for (int k = lane; k < N; k += 64) {
    const float wk = wr[k], g = lw[k], be = lb[k];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float h = (z2[(size_t)min(b0 + j, B - 1) * N + k] - st[0][j]) * st[1][j];
      acc[j] += silu_f(h * g + be) * wk;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0)
    for (int j = 0; j < 8 && b0 + j < B; ++j) {
      const float z = acc[j] + bias[n];
      if constexpr (STASH) z3[(size_t)(b0 + j) * N + n] = z;
      a3[(size_t)(b0 + j) * N + n] = silu_f(z);
    }
}
// ---- the x update (fv_head_set_flow_solver): explicit Runge-Kutta schemes whose stage j + 1 depends on stage j only; Euler is the one with a single stage.
// A higher-order step keeps two more rows per batch row, x0 (the step's start) and S (the running sum of b_j k_j).  Within a step of size h = dt, with k the
// stage's velocity (the corrected v' in the guided sampler) and xphi holding the stage's x:
//     first stage:      x0 <- x (xphi holds the step's start), S <- b k                 later stages:  S <- fmaf(b, k, S)
//     not the last:     x <- fmaf(a h, k, x0)                                           the last:      x <- fmaf(h, S, x0)
// ah = a_{j+1} h, b = b_j and h are rounded once on the host.  The lane or thread that owns (b, n) is the only one that touches x0, S and x of that element.
// A stage that is first AND last (Euler: b = 1) is x <- fmaf(h, k, x) and touches neither row: x0 and S may be null
struct FlowRkArgs { float* x0; float* S; float ah, b, h; int first, last; };
// every x + h k and x scale + shift of the samplers is ONE explicit fused multiply-add: equal operands give equal bits in all three
__device__ __forceinline__ float flow_fma_pinned(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// e = b N + n; xb = xphi[b][n] as it stands; -> the value xphi[b][n] takes.  ONE helper for all three samplers: equal k give equal bits.
// SINGLE: the caller's compile-time promise that the stage is first and last (the one-stage scheme), in both kernels that call this.  The same expressions,
// minus the branches on the two flags: in step C's serial epilogue they cost the prefix sampler 0.8 % at B = 64 (profiles/flow_refactor_ab.json)
template <bool SINGLE>
__device__ __forceinline__ float flow_rk_stage(const FlowRkArgs& rk, size_t e, float xb, float k) {
  const bool first = SINGLE || rk.first, last = SINGLE || rk.last;
  const float x0v = first ? xb : rk.x0[e];
  const float sv = first ? rk.b * k : flow_fma_pinned(rk.b, k, rk.S[e]);
  if (last) return flow_fma_pinned(rk.h, sv, x0v);
  if (first) rk.x0[e] = x0v;
  rk.S[e] = sv;
  return flow_fma_pinned(rk.ah, k, x0v);
}
// step kernel C: k = ba[n] + Wa[n] . a3[b]; x <- flow_rk_stage(x, k) in the epilogue (the lane that owns (b, n) reads and writes x[b][n], nobody else touches
// it).  t_next is the time of the NEXT evaluation (the next stage's, or the next step's first): unless this is the final one, the blocks of column group 0
// also write phi(t_next) for their 8 rows.  `actions` is given on the last stage of the last step only, which writes it (with the folded action statistics) and
// chunk_out (without, may be null).  PREFIX: a pinned element is left alone in xphi at every stage and never enters x0 or S; the final stage writes it out
// from x as it stands.  SINGLE: the instance for the one-stage scheme (flow_rk_stage)
template <bool PREFIX, bool SINGLE>
__global__ __launch_bounds__(256) void flow_step_c_kernel(const float* __restrict__ a3, int K, const float* __restrict__ W, const float* __restrict__ bias,
                                                           float* __restrict__ xphi, int xw, int te, FlowRkArgs rk, float t_next, const float* __restrict__ freq,
                                                           float* __restrict__ actions, float* __restrict__ chunk_out, const float* __restrict__ post_scale,
                                                           const float* __restrict__ post_shift, int B, int N, FlowPinned p) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), b0 = blockIdx.y * 8;
  if (!actions && blockIdx.x == 0) {
    const int half = te / 2;
    for (int idx = threadIdx.x; idx < 8 * half; idx += 256) {
      const int j = idx / half, i = idx - j * half;
      if (b0 + j < B) flow_phi(xphi + (size_t)(b0 + j) * xw + N, freq, half, t_next, i);
    }
  }
  if (n >= N) return;
  // this column's x (and the rows' pinned step counts) are asked for ahead of the product: their latency hides behind it instead of trailing the wave sums
  int pin[8];
  float xv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int b = min(b0 + j, B - 1);
    if constexpr (PREFIX) pin[j] = flow_pinned_steps(p, b);
    xv[j] = xphi[(size_t)b * xw + n];
  }
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  flow_dot8(a3, K, W + (size_t)n * K, K, b0, B, lane, acc);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0) {
    int k = 0;
    if constexpr (PREFIX) k = n / (N / p.chunk);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (b0 + j >= B) break;
      const size_t b = (size_t)(b0 + j);
      bool pinned = false;
      if constexpr (PREFIX) pinned = k < pin[j];
      const float xn = pinned ? xv[j] : flow_rk_stage<SINGLE>(rk, b * N + n, xv[j], acc[j] + bias[n]);
      if (!actions) {
        if (!pinned) xphi[b * xw + n] = xn;
        continue;
      }
      if (chunk_out) chunk_out[b * N + n] = xn;
      actions[b * N + n] = post_scale ? flow_fma_pinned(xn, post_scale[n], post_shift[n]) : xn;
    }
  }
}

// ---- guided sampling (fv_head_set_flow_guidance; real-time chunking).  Per step, with a^ = x - t v the denoised estimate, Y the shifted previous chunk and
// w >= 0 the per-step weights:   omega = w (Y - a^)    g = omega - t J^T omega  (J = dv / dx)    v' = v - k g    x <- x + dt v'
// The forward keeps the unguided kernels (A as it is, B with z3 kept, C' below in step C's order); J^T omega runs backwards through action_head, SiLU,
// fusion.4, SiLU, LayerNorm and the x columns of fusion.0.  Rows never meet: a row with omega == 0 gets g == 0 and v' == v exactly.
constexpr int FLOW_VJP_ROWS_MAX = 128;   // the largest reduction range of one block of flow_vjp_t_kernel
__device__ __forceinline__ float silu_grad_f(float z) {
  const float sg = sigmoid_f(z);
  return sg * (1.0f + z * (1.0f - sg));   // silu_bwd_kernel's expression
}
// step kernel C': v = ba[n] + Wa[n] . a3[b] in flow_step_c_kernel's order, kept in v_out; x stays.  step_w != null: omega as well.  Element (b, n) of step
// k = n / A: target prev[b][n + shift A] when k + shift < chunk.  A weight of 0, a step beyond the shift and a row with row_mask[b] == 0 are SELECTED to
// omega = 0: whatever prev holds there (NaN, +-inf) is never read into the arithmetic
__global__ __launch_bounds__(256) void flow_guide_c_kernel(const float* __restrict__ a3, int K, const float* __restrict__ W, const float* __restrict__ bias,
                                                            const float* __restrict__ xphi, int xw, float t, const float* __restrict__ prev,
                                                            const float* __restrict__ step_w, const int32_t* __restrict__ row_mask, int chunk, int A, int shift,
                                                            float* __restrict__ v_out, float* __restrict__ omega, int B, int N) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), b0 = blockIdx.y * 8;
  if (n >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  flow_dot8(a3, K, W + (size_t)n * K, K, b0, B, lane, acc);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0) {
    const int k = n / A;
    const float wk = step_w && k + shift < chunk ? step_w[k] : 0.f;
    for (int j = 0; j < 8 && b0 + j < B; ++j) {
      const size_t b = (size_t)(b0 + j);
      const float v = acc[j] + bias[n];
      v_out[b * N + n] = v;
      if (step_w) {
        float om = 0.f;
        if (wk != 0.f && (!row_mask || row_mask[b] != 0)) om = wk * (prev[b * N + n + (size_t)shift * A] - (xphi[b * xw + n] - t * v));
        omega[b * N + n] = om;
      }
    }
  }
}
// A transposed product on the row-major weight as it is stored: part[z][b][m] = sum over the block's range of n of g[b][n] W[n][col0 + m].  Lanes run along m
// (64 consecutive floats of a weight row per wave load), the block's `rps` reduction rows are dealt to its four waves (wave w: rows w, w + 4, ...), the four
// sums are folded through LDS in wave order, and blockIdx.z ranges of rps rows each write a partial of their own, which the NEXT kernel folds in z order:
// every sum has a fixed order, and at B = 1 the weight stream is spread over cdiv(M, 64) x cdiv(N, rps) blocks.
// The block first stages g for its 8 batch rows x rps reduction rows (rows beyond B: 0):
//   FOLD == 0: g = gin (B, ldg)           FOLD == 1: g = silu'(z[b][n]) * sum_q gin[q][b][n]  (gin: S_in partials of the previous product, (S_in, B, ldg))
template <int FOLD>
__global__ __launch_bounds__(256) void flow_vjp_t_kernel(const float* __restrict__ gin, int ldg, int S_in, const float* __restrict__ z,
                                                          const float* __restrict__ W, int ldw, int col0, float* __restrict__ part, int B, int N, int M, int rps) {
  __shared__ float gs[8][FLOW_VJP_ROWS_MAX];
  __shared__ float red[3][8][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m = blockIdx.x * 64 + lane, b0 = blockIdx.y * 8, n0 = blockIdx.z * rps;
  const int nn = min(rps, N - n0);
  for (int idx = threadIdx.x; idx < 8 * rps; idx += 256) {
    const int j = idx / rps, r = idx - j * rps, b = b0 + j, n = n0 + r;
    float val = 0.f;
    if (r < nn && b < B) {
      if constexpr (FOLD == 0) {
        val = gin[(size_t)b * ldg + n];
      } else {
        float sum = 0.f;
#pragma unroll 8
        for (int q = 0; q < S_in; ++q) sum += gin[((size_t)q * B + b) * ldg + n];
        val = sum * silu_grad_f(z[(size_t)b * ldg + n]);
      }
    }
    gs[j][r] = val;
  }
  __syncthreads();
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (m < M) {
    const float* wc = W + (size_t)n0 * ldw + col0 + m;
    for (int r = wv; r < nn; r += 4) {
      const float wk = wc[(size_t)r * ldw];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += gs[j][r] * wk;
    }
  }
  if (wv > 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wv - 1][j][lane] = acc[j];
  }
  __syncthreads();
  if (wv == 0 && m < M)
    for (int j = 0; j < 8 && b0 + j < B; ++j)
      part[((size_t)blockIdx.z * B + (b0 + j)) * M + m] = ((acc[j] + red[0][j][lane]) + red[1][j][lane]) + red[2][j][lane];
}
// LayerNorm backward of one row per block: dn2 = silu'(n2) * sum_q part[q][b][n] (the fusion.4 product's partials, folded in q order), dh = dn2 * gain,
// dz2 = rstd (dh - mean(dh) - h mean(dh h)).  The row's statistics are recomputed from z2 (ln_fwd_kernel's two passes); block sums go wave by wave
__device__ __forceinline__ float flow_block_sum(float v, float (&red)[16]) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}
// (256 or 1024 threads: at B = 1 this is ONE block, and what it waits for is the latency of the fold's loads -- a wide row gets a thread per element)
__global__ __launch_bounds__(1024) void flow_guide_ln_kernel(const float* __restrict__ z2, const float* __restrict__ lw, const float* __restrict__ lb,
                                                             const float* __restrict__ part, int S_in, float* __restrict__ dz2, int B, int N) {
  __shared__ float red[16];
  const int b = blockIdx.x, nt = blockDim.x;
  const float* zr = z2 + (size_t)b * N;
  float* dr = dz2 + (size_t)b * N;
  float s = 0.f;
  for (int i = threadIdx.x; i < N; i += nt) s += zr[i];
  const float mean = flow_block_sum(s, red) / (float)N;
  float q = 0.f;
  for (int i = threadIdx.x; i < N; i += nt) { const float d = zr[i] - mean; q += d * d; }
  const float rs = rsqrtf(flow_block_sum(q, red) / (float)N + LN_EPS);
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < N; i += nt) {
    const float h = (zr[i] - mean) * rs;
    float sum = 0.f;
#pragma unroll 8
    for (int p = 0; p < S_in; ++p) sum += part[((size_t)p * B + b) * N + i];
    const float dh = sum * silu_grad_f(h * lw[i] + lb[i]) * lw[i];
    dr[i] = dh;   // (read back by the same thread below)
    s1 += dh;
    s2 += dh * h;
  }
  const float m1 = flow_block_sum(s1, red) / (float)N, m2 = flow_block_sum(s2, red) / (float)N;
  for (int i = threadIdx.x; i < N; i += nt) {
    const float h = (zr[i] - mean) * rs;
    dr[i] = rs * (dr[i] - m1 - h * m2);
  }
}
// The last kernel of a guided evaluation, one thread per (b, n): J^T omega = sum_q part[q][b][n] (the fusion.0 product's partials), g = omega - t J^T omega,
// v' = v - kw g with t and kw the STAGE's, x <- flow_rk_stage(x, v'); phi(t_next), or on the final stage `actions` (with the folded statistics) and chunk_out
// (without), as flow_step_c_kernel: with v' == v it repeats step C's bits.  jt_out != null (the op-level entry): J^T omega alone.  SINGLE: as in step C
template <bool SINGLE>
__global__ __launch_bounds__(256) void flow_guide_update_kernel(const float* __restrict__ part, int S_in, const float* __restrict__ omega, const float* __restrict__ v,
                                                                 float* __restrict__ xphi, int xw, int te, float t, float kw, FlowRkArgs rk, float t_next,
                                                                 const float* __restrict__ freq, float* __restrict__ actions, float* __restrict__ chunk_out,
                                                                 const float* __restrict__ post_scale, const float* __restrict__ post_shift,
                                                                 float* __restrict__ jt_out, int B, int N) {
  const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (!jt_out && !actions && blockIdx.x == 0)
    for (int i = threadIdx.x; i < te / 2; i += 256) flow_phi(xphi + (size_t)b * xw + N, freq, te / 2, t_next, i);
  if (n >= N) return;
  const size_t e = (size_t)b * N + n;
  float jt = 0.f;
#pragma unroll 8
  for (int q = 0; q < S_in; ++q) jt += part[((size_t)q * B + b) * N + n];
  if (jt_out) { jt_out[e] = jt; return; }
  const float g = omega[e] - t * jt;
  const float vp = v[e] - kw * g;
  const float xn = flow_rk_stage<SINGLE>(rk, e, xphi[(size_t)b * xw + n], vp);
  if (!actions) { xphi[(size_t)b * xw + n] = xn; return; }
  if (chunk_out) chunk_out[e] = xn;
  actions[e] = post_scale ? flow_fma_pinned(xn, post_scale[n], post_shift[n]) : xn;
}

// the tableaux, indexed by FV_FLOW_SOLVER_*: stage times c, a[j] the coefficient that forms stage j + 1's x from k_j, b
struct FlowTableau { int stages; double c[4], a[3], b[4]; };
constexpr FlowTableau FLOW_TABLEAUX[4] = {
    {1, {0.0}, {}, {1.0}},                                                                  // Euler
    {2, {0.0, 0.5}, {0.5}, {0.0, 1.0}},                                                     // midpoint
    {2, {0.0, 1.0}, {1.0}, {0.5, 0.5}},                                                     // Heun
    {4, {0.0, 0.5, 0.5, 1.0}, {0.5, 0.5, 1.0}, {1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0}},   // RK4
};
static_assert(FV_FLOW_SOLVER_EULER == 0 && FV_FLOW_SOLVER_MIDPOINT == 1 && FV_FLOW_SOLVER_HEUN == 2 && FV_FLOW_SOLVER_RK4 == 3, "FLOW_TABLEAUX is indexed by the solver");
// what stage j of step i of n_steps needs: its time t, the next evaluation's time, and the epilogue's scalars -- all formed in double and rounded once, so a
// stage with c = 1 sees the bits of t_{i + 1}; Euler's are t_i = 1 - i / N, t_{i + 1} and h = dt = -1 / N.  rows: null for Euler, which never reads them
struct FlowStage { float t, t_next; FlowRkArgs rk; bool final; };
FlowStage flow_stage(const FlowTableau& tb, int i, int j, int n_steps, float* rows, size_t row_floats) {
  auto time = [&](int step, double c) { return (float)(1.0 - ((double)step + c) / (double)n_steps); };
  const bool last = j + 1 == tb.stages;
  const double h = -1.0 / (double)n_steps;
  FlowStage st;
  st.t = time(i, tb.c[j]);
  st.t_next = last ? time(i + 1, 0.0) : time(i, tb.c[j + 1]);
  st.rk = FlowRkArgs{rows, rows ? rows + row_floats : nullptr, last ? 0.f : (float)(tb.a[j] * h), (float)tb.b[j], (float)h, j == 0, last};
  st.final = last && i + 1 == n_steps;
  return st;
}
inline size_t flow_rk_row_floats(const HeadDims& d, int B) { return ((size_t)B * d.da + 3) / 4 * 4; }
int flow_solver_check(const char* who, int solver, const float* rk_rows) {
  if (solver < FV_FLOW_SOLVER_EULER || solver > FV_FLOW_SOLVER_RK4) return fv_fail(FV_ERR_ARG, "%s: unknown solver %d", who, solver);
  if (solver != FV_FLOW_SOLVER_EULER && !rk_rows) return fv_fail(FV_ERR_STATE, "%s: a higher-order solver needs its rows (fv_head_set_flow_solver before fv_bind_workspace)", who);
  return FV_OK;
}
// The one loop of every sampler, n_steps x stages network evaluations: eval(stage, out) issues the sampler's launches for one of them.  `out` is where the
// final stage writes the result -- all null before it, so its kernel writes phi(t_next) instead
struct FlowOut { float *actions, *chunk_out; const float *post_scale, *post_shift; };
template <class Eval>
void flow_integrate(const HeadDims& d, int B, int n_steps, int solver, float* rk_rows, float* actions, float* chunk_out, const HeadIoNorm* io, Eval&& eval) {
  const FlowTableau& tb = FLOW_TABLEAUX[solver];
  for (int i = 0; i < n_steps; ++i)
    for (int j = 0; j < tb.stages; ++j) {
      const FlowStage st = flow_stage(tb, i, j, n_steps, rk_rows, flow_rk_row_floats(d, B));
      eval(st, st.final ? FlowOut{actions, chunk_out, io ? io->action_std : nullptr, io ? io->action_mean : nullptr} : FlowOut{});
    }
}

}  // namespace

size_t flow_rk_scratch_bytes(const HeadDims& d, int B) { return d.te > 0 ? 2 * flow_rk_row_floats(d, B) * sizeof(float) : 0; }

int launch_flow_prepare(const HeadDims& d, const HeadFlow& f, const float* targets, int B, uint64_t seed, uint64_t offset, const float* noise, const float* t,
                        float* saved, float* u_out, hipStream_t s, const int32_t* delays) {
  if (d.te <= 0 || !f.freq) return fv_fail(FV_ERR_STATE, "flow_prepare: the head is not in flow mode (fv_head_set_flow)");
  if (delays && d.pk <= 0) return fv_fail(FV_ERR_STATE, "flow_prepare: delays need prefix mode (fv_head_set_flow_prefix)");
  if (d.pk > 0 && !delays && !f.thr) return fv_fail(FV_ERR_STATE, "flow_prepare: prefix mode without a delay table");
  if (!targets || !saved || !u_out) return fv_fail(FV_ERR_ARG, "flow_prepare: null pointer");
  if (B <= 0) return fv_fail(FV_ERR_ARG, "flow_prepare: B must be positive");
  const int S = head_rows(d, B) / B;
  if (S > 1 && (offset >> 56 & 15)) return fv_fail(FV_ERR_ARG, "flow_prepare: bits 56 .. 59 of the offset number the draws and must be 0 with more than one draw");
  const FlowPrefixArgs px = d.pk > 0 ? FlowPrefixArgs{delays, f.thr, head_saved_prefix_mask(d, B, saved), d.pk, d.pd} : FlowPrefixArgs{};
  // fv_head_set_flow_time: the handle's own distribution gives way to the setting's.  The TIMED instances run only where the setting changes a drawn t: a
  // Beta, a range other than [0, 1], or strata with more than one draw; explicit t, and a setting that amounts to uniform or logit-normal on [0, 1], launch
  // the plain instances with the plain arguments
  const FlowTime& tm = f.tm;
  const int dist = tm.on ? tm.dist : f.time_dist;
  const float da_ = tm.on ? tm.a : f.dist_a, db_ = tm.on ? tm.b : f.dist_b;
  const int strat = tm.on && tm.stratify && S > 1;
  const bool timed = tm.on && !t && (dist == 2 || strat || tm.t_lo != 0.f || tm.t_hi != 1.f);
  const FlowTimeArgs ta{dist, strat, (double)tm.a, (double)tm.b, tm.lbeta, (double)tm.t_lo, (double)tm.t_hi - (double)tm.t_lo};
  if (timed) {
    const auto kern = d.pk > 0 ? flow_prepare_kernel<true, FlowTimeArgs> : flow_prepare_kernel<false, FlowTimeArgs>;
    hipLaunchKernelGGL(kern, dim3(B, S), dim3(256), 0, s, targets, noise, t, head_saved_cat(d, B, saved), head_cat_width(d), d.feat + d.hid, u_out, d.da, d.te, f.freq,
                       dist, da_, db_, seed, offset, px, ta);
  } else
    hipLaunchKernelGGL(d.pk > 0 ? flow_prepare_kernel<true> : flow_prepare_kernel<false>, dim3(B, S), dim3(256), 0, s, targets, noise, t, head_saved_cat(d, B, saved),
                       head_cat_width(d), d.feat + d.hid, u_out, d.da, d.te, f.freq, dist, da_, db_, seed, offset, px);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

namespace {
struct FlowScratch { float *n0, *xh0, *rstd0, *z1, *sb, *c, *xphi, *z2, *a3; size_t total; };
FlowScratch flow_carve(const HeadDims& d, int B, float* base) {
  FlowScratch r;
  size_t o = 0;
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += (n + 3) / 4 * 4; return p; };
  r.n0 = take((size_t)B * d.ds); r.xh0 = take((size_t)B * d.ds); r.rstd0 = take(B); r.z1 = take((size_t)B * d.hid); r.sb = take((size_t)B * d.hid);
  r.c = take((size_t)B * d.fus); r.xphi = take((size_t)B * (d.da + d.te)); r.z2 = take((size_t)B * d.fus); r.a3 = take((size_t)B * d.fus);
  r.total = o;
  return r;
}
// the conditioning of a sampler call (4 launches): state LayerNorm, state projection, the t-independent part of fusion.0, the start [x | phi(t0)].
// pin != null: the PREFIX instances of the last two.  S > 1 (fv_head_flow_sample_multi; fs carved for S B rows): the state branch and c run on the B
// observations, one more launch copies c into the rows of candidates 1 .. S - 1, and the start writes all S B rows (delays_rows: its copy of the delays)
void flow_condition(const HeadDims& d, const HeadFlow& f, const HeadOffsets& ho, const FlowScratch& fs, const float* P, const float* pooled, const float* states,
                    int B, const float* noise, float t0, uint64_t seed, uint64_t offset, hipStream_t s, const HeadIoNorm* io, const FlowPinned* pin = nullptr,
                    int S = 1, int32_t* delays_rows = nullptr) {
  const dim3 blk(256);
  const FlowPinned p = pin ? *pin : FlowPinned{};
  launch_head_state_branch(d, P, states, B, fs.n0, fs.xh0, fs.rstd0, fs.z1, fs.sb, d.hid, s, io);
  hipLaunchKernelGGL(pin ? flow_cond_kernel<true> : flow_cond_kernel<false>, dim3(cdiv(d.fus, 4), cdiv(B, 8)), blk, 0, s, pooled, d.feat, fs.sb, d.hid, P + ho.o[HP_FUS0_W],
                     head_cat_width(d), P + ho.o[HP_FUS0_B], fs.c, B, d.fus, d.feat + d.hid + d.da + d.te, p);
  if (S > 1) hipLaunchKernelGGL(flow_cond_broadcast_kernel, dim3(cdiv((long)B * d.fus, 256), S - 1), blk, 0, s, fs.c, B, d.fus);
  hipLaunchKernelGGL(pin ? flow_init_kernel<true> : flow_init_kernel<false>, dim3(B, S), blk, 0, s, noise, fs.xphi, d.da, d.te, f.freq, t0, seed, offset, p, delays_rows);
}
// The launches of the plain and the prefix sampler, checks done: the conditioning on B observations, then three launches per network evaluation on R = S B
// head rows (S == 1: launch_flow_sample's, as ever).  io: the state statistics; io_out: the action statistics the final stage folds (null: normalised output).
// delays_rows (S > 1 with pin): R ints the start fills, which step C reads per head row in place of pin->delays
void flow_sample_rows(const HeadDims& d, const HeadFlow& f, const float* P, const float* pooled, const float* states, int B, int S, int n_steps, const float* noise,
                      uint64_t seed, uint64_t offset, float* actions, float* chunk_out, const FlowScratch& fs, hipStream_t s, const HeadIoNorm* io,
                      const HeadIoNorm* io_out, int solver, float* rk_rows, const FlowPin* pin, int32_t* delays_rows) {
  const HeadOffsets ho = head_offsets(d);
  const int cw = head_cat_width(d), xo = d.feat + d.hid, xw = d.da + d.te, R = S * B;
  const dim3 blk(256);
  const unsigned b8 = cdiv(R, 8);
  const FlowPinned p = pin ? FlowPinned{pin->prev, pin->delays, d.pd, d.pk, pin->shift} : FlowPinned{};
  FlowPinned pr = p;   // step C's: a delay per head row
  if (pin && S > 1) pr.delays = delays_rows;
  const bool single = FLOW_TABLEAUX[solver].stages == 1;
  const auto step_c = pin ? (single ? flow_step_c_kernel<true, true> : flow_step_c_kernel<true, false>) : (single ? flow_step_c_kernel<false, true> : flow_step_c_kernel<false, false>);
  flow_condition(d, f, ho, fs, P, pooled, states, B, noise, 1.0f, seed, offset, s, io, pin ? &p : nullptr, S, pin && S > 1 ? delays_rows : nullptr);
  flow_integrate(d, R, n_steps, solver, rk_rows, actions, chunk_out, io_out, [&](const FlowStage& st, const FlowOut& out) {
    hipLaunchKernelGGL(flow_step_a_kernel, dim3(cdiv(d.fus, 4), b8), blk, 0, s, fs.xphi, xw, P + ho.o[HP_FUS0_W], cw, xo, fs.c, fs.z2, R, d.fus);
    hipLaunchKernelGGL(flow_step_b_kernel<false>, dim3(cdiv(d.fus, 4), b8), blk, 0, s, fs.z2, P + ho.o[HP_FUS_LN_W], P + ho.o[HP_FUS_LN_B], P + ho.o[HP_FUS4_W], P + ho.o[HP_FUS4_B], fs.a3,
                       (float*)nullptr, R, d.fus);
    hipLaunchKernelGGL(step_c, dim3(cdiv(d.da, 4), b8), blk, 0, s, fs.a3, d.fus, P + ho.o[HP_ACT_W], P + ho.o[HP_ACT_B], fs.xphi, xw,
                       d.te, st.rk, st.t_next, f.freq, out.actions, out.chunk_out, out.post_scale, out.post_shift, R, d.da, pr);
  });
}
}  // namespace

size_t flow_sample_scratch_bytes(const HeadDims& d, int B) { return d.te > 0 ? flow_carve(d, B, nullptr).total * sizeof(float) : 0; }

// 4 launches of conditioning, then 3 per network evaluation.  No dropout, no atomics, no host synchronisation; every time and step size is rounded once on
// the host and travels as a kernel argument.  pin != null: the prefix sampler (the conditioning's, the start's and step C's PREFIX instances)
int launch_flow_sample(const HeadDims& d, const HeadFlow& f, const float* P, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                       uint64_t seed, uint64_t offset, float* actions, float* scratch, hipStream_t s, const HeadIoNorm* io, int solver, float* rk_rows,
                       const FlowPin* pin) {
  const char* who = pin ? "flow_sample_prefix" : "flow_sample";
  if (d.te <= 0 || !f.freq) return fv_fail(FV_ERR_STATE, "%s: the head is not in flow mode (fv_head_set_flow)", who);
  if (pin && (d.pk < 2 || d.da % d.pk || d.pd < 1 || d.pd >= d.pk)) return fv_fail(FV_ERR_STATE, "%s: prefix mode is off (fv_head_set_flow_prefix)", who);
  if (!P || !pooled || !states || (pin && (!pin->prev || !pin->delays)) || !actions || !scratch) return fv_fail(FV_ERR_ARG, "%s: null pointer", who);
  if (B <= 0 || n_steps < 1) return fv_fail(FV_ERR_ARG, "%s: B and n_steps must be positive", who);
  if (pin && (pin->shift < 0 || pin->shift > d.pk)) return fv_fail(FV_ERR_ARG, "%s: shift = %d outside 0 .. chunk = %d", who, pin->shift, d.pk);
  if (const int rc = flow_solver_check(who, solver, rk_rows)) return rc;
  flow_sample_rows(d, f, P, pooled, states, B, 1, n_steps, noise, seed, offset, actions, pin ? pin->chunk_out : nullptr, flow_carve(d, B, scratch), s, io, io, solver, rk_rows,
                   pin, nullptr);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

namespace {
// the rows of a multi-sample call: the sampler's for S B head rows, then the S B normalised candidates and, for the prefix sampler, a delay per head row
struct MultiScratch { FlowScratch fs; float* cand; int32_t* delays; size_t total; };
MultiScratch multi_carve(const HeadDims& d, int R, float* base) {
  MultiScratch r;
  r.fs = flow_carve(d, R, base);
  size_t o = r.fs.total;
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += (n + 3) / 4 * 4; return p; };
  r.cand = take((size_t)R * d.da);
  r.delays = reinterpret_cast<int32_t*>(take(R));
  r.total = o;
  return r;
}
}  // namespace

size_t flow_multi_scratch_bytes(const HeadDims& d, int R) { return d.te > 0 ? multi_carve(d, R, nullptr).total * sizeof(float) : 0; }

// S candidates per observation in one call, then the choice among them (flow_select_kernels.hip).  The conditioning runs on B rows and is copied, the steps
// run unchanged on S B rows -- at B = 1 up to eight candidates share the one pass flow_dot8 makes anyway --, the final stage writes the normalised
// candidates into scratch without the folded statistics, and the selection kernel writes every output.  pin != null: the candidates of the prefix sampler
int launch_flow_sample_multi(const HeadDims& d, const HeadFlow& f, const float* P, const float* pooled, const float* states, int B, int S, int n_steps,
                             const float* noise, uint64_t seed, uint64_t offset, float* scratch, hipStream_t s, const HeadIoNorm* io, int solver, float* rk_rows,
                             const FlowPin* pin, const FlowSelect& sel) {
  const char* who = "flow_sample_multi";
  if (d.te <= 0 || !f.freq) return fv_fail(FV_ERR_STATE, "%s: the head is not in flow mode (fv_head_set_flow)", who);
  if (pin && (d.pk < 2 || d.da % d.pk || d.pd < 1 || d.pd >= d.pk)) return fv_fail(FV_ERR_STATE, "%s: prefix mode is off (fv_head_set_flow_prefix)", who);
  if (!P || !pooled || !states || (pin && (!pin->prev || !pin->delays)) || !scratch) return fv_fail(FV_ERR_ARG, "%s: null pointer", who);
  if (B <= 0 || n_steps < 1) return fv_fail(FV_ERR_ARG, "%s: B and n_steps must be positive", who);
  if (S < 1 || S > FV_FLOW_SAMPLES_MAX) return fv_fail(FV_ERR_ARG, "%s: S = %d outside 1 .. %d", who, S, FV_FLOW_SAMPLES_MAX);
  if (S > 1 && (offset >> 56 & 15)) return fv_fail(FV_ERR_ARG, "%s: bits 56 .. 59 of the offset number the candidates and must be 0 with more than one", who);
  if (pin && (pin->shift < 0 || pin->shift > d.pk)) return fv_fail(FV_ERR_ARG, "%s: shift = %d outside 0 .. chunk = %d", who, pin->shift, d.pk);
  if (const int rc = flow_solver_check(who, solver, rk_rows)) return rc;
  if (const int rc = flow_select_check(sel, S, d.da)) return rc;
  const MultiScratch ms = multi_carve(d, S * B, scratch);
  // one candidate and none of the optional outputs: there is nothing to choose and nothing to report, so the final stage writes actions and chunk_out
  // itself, as the prefix sampler always did -- the single-sample call's launches, no more
  if (S == 1 && !sel.candidates_out && !sel.choice_out && !sel.scores_out && !sel.spread_out) {
    flow_sample_rows(d, f, P, pooled, states, B, 1, n_steps, noise, seed, offset, sel.actions, sel.chunk_out, ms.fs, s, io, io, solver, rk_rows, pin, nullptr);
    FV_HIP_CHECK(hipGetLastError());
    return FV_OK;
  }
  // (S == 1 needs no row beyond the plain sampler's, so a handle that never grew its plan can make the call: the one candidate lands in chunk_out, where the
  // selection kernel reads it and writes it back, element by element in the thread that owns it)
  float* cand = S > 1 ? ms.cand : sel.chunk_out;
  flow_sample_rows(d, f, P, pooled, states, B, S, n_steps, noise, seed, offset, cand, nullptr, ms.fs, s, io, nullptr, solver, rk_rows, pin, ms.delays);
  return launch_flow_select(cand, B, S, d.da, sel, io ? io->action_std : nullptr, io ? io->action_mean : nullptr, s);
}

namespace {
// the guided sampler's rows: the unguided sampler's, then z3, v, omega, dz2 and two partial-sum buffers the transposed products alternate between
struct GuideScratch { FlowScratch fs; float *z3, *v, *omega, *dz2, *pa, *pb; size_t total; };
// k = min(beta, ((1 - t)^2 + t^2) / ((1 - t) t)) for a stage time: in double from the fp32-rounded t, rounded once; beta at t = 1 and, the ratio being unbounded
// there, at t = 0
inline float guide_weight(float t, float beta) {
  const double td = (double)t;
  return t >= 1.0f || t <= 0.0f ? beta : (float)std::min((double)beta, ((1.0 - td) * (1.0 - td) + td * td) / ((1.0 - td) * td));
}
inline int guide_rps(int B) { return B <= 16 ? 64 : FLOW_VJP_ROWS_MAX; }   // reduction rows per block: more, smaller ranges while few batch groups fill the chip
size_t guide_part_floats(const HeadDims& d, int B) {
  auto per_row = [&](int rps) {
    const size_t sa = cdiv(d.da, rps), sf = cdiv(d.fus, rps);
    return std::max(std::max(sa, sf) * (size_t)d.fus, sf * (size_t)d.da);
  };
  // (never smaller for a larger B: a call with B rows fits the workspace sized for max_batch)
  return B <= 16 ? (size_t)B * per_row(64) : std::max((size_t)16 * per_row(64), (size_t)B * per_row(FLOW_VJP_ROWS_MAX));
}
GuideScratch guide_carve(const HeadDims& d, int B, float* base) {
  GuideScratch r;
  r.fs = flow_carve(d, B, base);
  size_t o = r.fs.total;
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += (n + 3) / 4 * 4; return p; };
  r.z3 = take((size_t)B * d.fus); r.v = take((size_t)B * d.da); r.omega = take((size_t)B * d.da); r.dz2 = take((size_t)B * d.fus);
  r.pa = take(guide_part_floats(d, B)); r.pb = take(guide_part_floats(d, B));
  r.total = o;
  return r;
}
// forward of a guided step: A, B with z3 kept, C' (v, and omega when step_w is given)
void guide_forward(const HeadDims& d, const HeadOffsets& ho, const GuideScratch& g, const float* P, int B, float t, const float* prev, const float* step_w,
                   const int32_t* row_mask, int chunk, int shift, float* v_out, hipStream_t s) {
  const dim3 blk(256);
  const unsigned b8 = cdiv(B, 8);
  const int xw = d.da + d.te;
  hipLaunchKernelGGL(flow_step_a_kernel, dim3(cdiv(d.fus, 4), b8), blk, 0, s, g.fs.xphi, xw, P + ho.o[HP_FUS0_W], head_cat_width(d), d.feat + d.hid, g.fs.c, g.fs.z2, B, d.fus);
  hipLaunchKernelGGL(flow_step_b_kernel<true>, dim3(cdiv(d.fus, 4), b8), blk, 0, s, g.fs.z2, P + ho.o[HP_FUS_LN_W], P + ho.o[HP_FUS_LN_B], P + ho.o[HP_FUS4_W], P + ho.o[HP_FUS4_B], g.fs.a3, g.z3, B,
                     d.fus);
  hipLaunchKernelGGL(flow_guide_c_kernel, dim3(cdiv(d.da, 4), b8), blk, 0, s, g.fs.a3, d.fus, P + ho.o[HP_ACT_W], P + ho.o[HP_ACT_B], g.fs.xphi, xw, t, prev, step_w, row_mask,
                     chunk, d.da / chunk, shift, v_out, g.omega, B, d.da);
}
// J^T omega as partial sums: action_head^T over the first n_live rows (the steps behind them have omega == 0), fusion.4^T, LayerNorm, fusion.0[:, x]^T.
// -> the number of partials (B, da) left in g.pa, which flow_guide_update_kernel folds
int guide_backward(const HeadDims& d, const HeadOffsets& ho, const GuideScratch& g, const float* P, const float* omega, int n_live, int B, hipStream_t s) {
  const dim3 blk(256);
  const unsigned b8 = cdiv(B, 8);
  const int rps = guide_rps(B), sd = (int)cdiv(n_live, rps), sf = (int)cdiv(d.fus, rps);
  hipLaunchKernelGGL(flow_vjp_t_kernel<0>, dim3(cdiv(d.fus, 64), b8, sd), blk, 0, s, omega, d.da, 0, (const float*)nullptr, P + ho.o[HP_ACT_W], d.fus, 0, g.pa, B, n_live,
                     d.fus, rps);
  hipLaunchKernelGGL(flow_vjp_t_kernel<1>, dim3(cdiv(d.fus, 64), b8, sf), blk, 0, s, g.pa, d.fus, sd, g.z3, P + ho.o[HP_FUS4_W], d.fus, 0, g.pb, B, d.fus, d.fus, rps);
  hipLaunchKernelGGL(flow_guide_ln_kernel, dim3(B), dim3(d.fus >= 1024 ? 1024 : 256), 0, s, g.fs.z2, P + ho.o[HP_FUS_LN_W], P + ho.o[HP_FUS_LN_B], g.pb, sf, g.dz2, B, d.fus);
  hipLaunchKernelGGL(flow_vjp_t_kernel<0>, dim3(cdiv(d.da, 64), b8, sf), blk, 0, s, g.dz2, d.fus, 0, (const float*)nullptr, P + ho.o[HP_FUS0_W], head_cat_width(d),
                     d.feat + d.hid, g.pa, B, d.fus, d.da, rps);
  return sf;
}
}  // namespace

size_t flow_guided_scratch_bytes(const HeadDims& d, int B) { return d.te > 0 ? guide_carve(d, B, nullptr).total * sizeof(float) : 0; }

// Conditioning as launch_flow_sample, then 8 launches per network evaluation, each guided at the STAGE's time: A, B (z3 kept), C' (v and omega), three
// transposed products with a LayerNorm backward between the last two, and the update.  The stage's times and weight, the step size, shift and the live-row
// count are host values that travel as kernel arguments
int launch_flow_sample_guided(const HeadDims& d, const HeadFlow& f, const HeadGuide& gd, const float* P, const float* pooled, const float* states, int B, int n_steps,
                              const float* noise, uint64_t seed, uint64_t offset, const float* prev, int shift, const int32_t* row_mask, float* actions,
                              float* chunk_out, float* scratch, hipStream_t s, const HeadIoNorm* io, int solver, float* rk_rows) {
  if (d.te <= 0 || !f.freq) return fv_fail(FV_ERR_STATE, "flow_sample_guided: the head is not in flow mode (fv_head_set_flow)");
  if (!gd.step_w || gd.chunk < 1 || d.da % gd.chunk) return fv_fail(FV_ERR_STATE, "flow_sample_guided: guidance is not configured (fv_head_set_flow_guidance)");
  if (!P || !pooled || !states || !prev || !actions || !scratch) return fv_fail(FV_ERR_ARG, "flow_sample_guided: null pointer");
  if (B <= 0 || n_steps < 1) return fv_fail(FV_ERR_ARG, "flow_sample_guided: B and n_steps must be positive");
  if (shift < 0 || shift > gd.chunk) return fv_fail(FV_ERR_ARG, "flow_sample_guided: shift = %d outside 0 .. chunk = %d", shift, gd.chunk);
  if (const int rc = flow_solver_check("flow_sample_guided", solver, rk_rows)) return rc;
  const HeadOffsets ho = head_offsets(d);
  const GuideScratch g = guide_carve(d, B, scratch);
  const int A = d.da / gd.chunk, xw = d.da + d.te;
  // steps from here on have omega == 0 (weight 0, or beyond the shift): the first product stops there.  (At least one step: its omega is then all 0)
  const int n_live = std::max(1, std::min(gd.live_steps, gd.chunk - shift)) * A;
  flow_condition(d, f, ho, g.fs, P, pooled, states, B, noise, 1.0f, seed, offset, s, io);
  const auto update = FLOW_TABLEAUX[solver].stages == 1 ? flow_guide_update_kernel<true> : flow_guide_update_kernel<false>;
  flow_integrate(d, B, n_steps, solver, rk_rows, actions, chunk_out, io, [&](const FlowStage& st, const FlowOut& out) {
    guide_forward(d, ho, g, P, B, st.t, prev, gd.step_w, row_mask, gd.chunk, shift, g.v, s);
    const int sp = guide_backward(d, ho, g, P, g.omega, n_live, B, s);
    hipLaunchKernelGGL(update, dim3(cdiv(d.da, 256), B), dim3(256), 0, s, g.pa, sp, g.omega, g.v, g.fs.xphi, xw, d.te, st.t, guide_weight(st.t, gd.beta), st.rk,
                       st.t_next, f.freq, out.actions, out.chunk_out, out.post_scale, out.post_shift, (float*)nullptr, B, d.da);
  });
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

// one guided step's chain for a given x, t and omega (tests): v (B, da) and J^T omega (B, da)
int launch_flow_vjp(const HeadDims& d, const HeadFlow& f, const float* P, const float* pooled, const float* states, int B, const float* x, float t,
                    const float* omega, float* v_out, float* jt_out, float* scratch, hipStream_t s) {
  if (d.te <= 0 || !f.freq) return fv_fail(FV_ERR_STATE, "flow_vjp: the head is not in flow mode");
  if (!P || !pooled || !states || !x || !omega || !v_out || !jt_out || !scratch) return fv_fail(FV_ERR_ARG, "flow_vjp: null pointer");
  if (B <= 0) return fv_fail(FV_ERR_ARG, "flow_vjp: B must be positive");
  const HeadOffsets ho = head_offsets(d);
  const GuideScratch g = guide_carve(d, B, scratch);
  flow_condition(d, f, ho, g.fs, P, pooled, states, B, x, t, 0, 0, s, nullptr);
  guide_forward(d, ho, g, P, B, t, nullptr, nullptr, nullptr, 1, 0, v_out, s);
  const int sp = guide_backward(d, ho, g, P, omega, d.da, B, s);
  hipLaunchKernelGGL(flow_guide_update_kernel<true>, dim3(cdiv(d.da, 256), B), dim3(256), 0, s, g.pa, sp, omega, v_out, g.fs.xphi, d.da + d.te, d.te, t, 0.f, FlowRkArgs{}, 0.f,
                     f.freq, (float*)nullptr, (float*)nullptr, (const float*)nullptr, (const float*)nullptr, jt_out, B, d.da);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

}  // namespace fv
