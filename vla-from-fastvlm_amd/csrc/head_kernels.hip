// head_kernels.hip -- the action expert itself, the only trainable part of the frozen-backbone path, all fp32 (the reference keeps it fp32 too):
//   forward                     reference fastvla/fastvlm_with_expert.py:23-38,50-54; the state branch alone (launch_head_state_branch) also serves the samplers
//   MSE + hand-derived backward for the 12 head tensors (kernels.h HeadParam)   fastvla/modeling_fastvla.py:56, trainer.py:175
//   the layout of the flat parameter buffer (head_offsets) and of the saved activations (Saved / carve)
//   several noise draws per observation (fv_head_set_flow_draws): the three draws_* kernels between the state branch and fusion.0, forward and backward
// Its neighbours: chunk_kernels.hip (the chunked losses and the ensembling ring), flow_kernels.hip (the flow head's preparation and both samplers),
// optim_kernels.hip (clip + AdamW, single-group and grouped, and axpy).
// 3.05 M parameters / ~18 MFLOP per sample: launch-latency bound, so the kernels are simple wave-per-output fp32
// dot products with coalesced weight reads; parameters and gradients are views into flat caller-owned buffers.
#include "kernels.h"

namespace fv {
namespace {

// one wave per row: y = LN(x) * w + b, saves xhat and rstd
// pre_mean / pre_istd (may be null): the dataset normalisation of the input folded in, x <- (x - pre_mean) * pre_istd
// (LeRobot NormalizerProcessorStep, MEAN_STD; reference lerobot_fastvla/processor_fastvla.py:34-39)
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ y,
                                                      float* __restrict__ xhat, float* __restrict__ rstd, int rows, int n,
                                                      const float* __restrict__ pre_mean, const float* __restrict__ pre_istd) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * ldx;
  auto in = [&](int i) { return pre_mean ? (xr[i] - pre_mean[i]) * pre_istd[i] : xr[i]; };
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s += in(i);
  const float mean = wave_sum(s) / (float)n;
  float q = 0.f;
  for (int i = lane; i < n; i += 64) { const float d = in(i) - mean; q += d * d; }
  const float rs = rsqrtf(wave_sum(q) / (float)n + LN_EPS);
  for (int i = lane; i < n; i += 64) {
    const float h = (in(i) - mean) * rs;
    xhat[(size_t)row * n + i] = h;
    y[(size_t)row * n + i] = h * w[i] + b[i];
  }
  if (lane == 0) rstd[row] = rs;
}

// y[b][n] = sum_k x[b][k] W[n][k] + bias[n]; one wave per n, 8 batch rows per pass.  act 1: z = pre-activation,
// y = silu(z).  y may be a strided view (ldy) -- the state branch writes straight into cat[:, feat:].
__global__ __launch_bounds__(256) void linear_fwd_kernel(const float* __restrict__ x, int ldx,
                                                          const float* __restrict__ W, const float* __restrict__ bias,
                                                          float* __restrict__ y, int ldy, float* __restrict__ z, int B,
                                                          int N, int K, int act, const float* __restrict__ post_scale,
                                                          const float* __restrict__ post_shift) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b0 = blockIdx.y * 8;
  if (n >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const float* wr = W + (size_t)n * K;
  for (int k = lane; k < K; k += 64) {
    const float wv = wr[k];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += x[(size_t)min(b0 + j, B - 1) * ldx + k] * wv;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0) {
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (b0 + j >= B) break;
      const float v = acc[j] + bv;
      if (act) { z[(size_t)(b0 + j) * N + n] = v; y[(size_t)(b0 + j) * ldy + n] = silu_f(v); }
      else y[(size_t)(b0 + j) * ldy + n] = post_scale ? v * post_scale[n] + post_shift[n] : v;   // action un-normalisation folded in
    }
  }
}

// dx[b][k] = sum_n dy[b][n] W[n][k].  Block = 32 k x 8 batch rows; its 256 threads are 8 n-lanes x 32 k: lane j sums n = j, j + 8, ... (N / 8
// steps instead of N: the first version's 32 blocks of N-long dependent loops took 196 us per call at B = 32, N = 1024, K = 1920 -- 3 % of
// the C3 rank-shape train step for 126 MFLOP), the eight partial sums are folded through LDS in a fixed order (bit-repeatable).
__global__ __launch_bounds__(256) void linear_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ W,
                                                             float* __restrict__ dx, int lddx, int B, int N, int K) {
  __shared__ float part[8][8][32];   // [n-lane][batch row][k]
  const int tid = threadIdx.x, kl = tid & 31, nl = tid >> 5;
  const int k = blockIdx.x * 32 + kl, kc = min(k, K - 1);
  const int b0 = blockIdx.y * 8;
  const float* dyr[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dyr[j] = dy + (size_t)min(b0 + j, B - 1) * N;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
  for (int n = nl; n < N; n += 8) {
    const float wv = W[(size_t)n * K + kc];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += dyr[j][n] * wv;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[nl][j][kl] = acc[j];
  __syncthreads();
  const int j = tid >> 5;   // one (batch row, k) per thread
  float sum = 0.f;
#pragma unroll
  for (int l = 0; l < 8; ++l) sum += part[l][j][kl];
  if (k < K && b0 + j < B) dx[(size_t)(b0 + j) * lddx + k] = sum;
}

// dW[n][k] = sum_b dy[b][n] x[b][k]; block = one n, 256 k
__global__ __launch_bounds__(256) void linear_bwd_dw_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                             int ldx, float* __restrict__ dW, int B, int N, int K) {
  const int k = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (k >= K) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc += dy[(size_t)b * N + n] * x[(size_t)b * ldx + k];
  dW[(size_t)n * K + k] = acc;
}

__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ dy, float* __restrict__ db, int B, int N) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc += dy[(size_t)b * N + n];
  db[n] = acc;
}

// g <- silu'(z) * g * (mul ? mul : 1); src may be a strided view (ds = dcat[:, feat:])
__global__ __launch_bounds__(256) void silu_bwd_kernel(const float* __restrict__ gin, int ldg, const float* __restrict__ z,
                                                        const float* __restrict__ mul, float* __restrict__ gout, int B, int N) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * N) return;
  const int b = (int)(i / N), n = (int)(i % N);
  float g = gin[(size_t)b * ldg + n];
  if (mul) g *= mul[i];
  const float zz = z[i], sg = sigmoid_f(zz);
  gout[i] = g * sg * (1.0f + zz * (1.0f - sg));
}

// dropout after SiLU(LayerNorm): d2 = silu(n2) * keep/(1-p); mask holds the multiplier
__global__ __launch_bounds__(256) void silu_dropout_kernel(const float* __restrict__ n2, float* __restrict__ d2,
                                                            float* __restrict__ mask, long total, int training, float p,
                                                            uint64_t seed, uint64_t offset) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float mlt = 1.0f;
  if (training && p > 0.f) {
    const uint64_t ctr = (uint64_t)(i >> 2);
    const uint4 r = philox(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)),
                           make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    const uint32_t rv[4] = {r.x, r.y, r.z, r.w};
    const float u = (float)(rv[i & 3] >> 8) * (1.0f / 16777216.0f);
    mlt = u >= p ? 1.0f / (1.0f - p) : 0.f;
  }
  mask[i] = mlt;
  d2[i] = silu_f(n2[i]) * mlt;
}

__global__ __launch_bounds__(256) void copy_cols_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst,
                                                         int ldd, int B, int N) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * N) return;
  const int b = (int)(i / N), n = (int)(i % N);
  dst[(size_t)b * ldd + n] = src[(size_t)b * lds + n];
}

// single block: loss = mean((a-t)^2), g = 2 (a-t) / (B*A)
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ a, const float* __restrict__ t,
                                                   float* __restrict__ loss, float* __restrict__ g, int n, float loss_scale) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = a[i] - t[i];
    s += d * d;
    g[i] = loss_scale * 2.0f * d / (float)n;   // loss_scale (a power of two, 1 by default) scales every gradient downstream; the loss itself is not scaled
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (red[0] + red[1] + red[2] + red[3]) / (float)n;
}

// LN backward: wave per row -> dx (may be null); column sums dw, db done by ln_bwd_cols_kernel
__global__ __launch_bounds__(256) void ln_bwd_rows_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                           const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                           float* __restrict__ dx, int rows, int n) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float s1 = 0.f, s2 = 0.f;
  for (int i = lane; i < n; i += 64) {
    const float g = dy[(size_t)row * n + i] * w[i];
    s1 += g;
    s2 += g * xhat[(size_t)row * n + i];
  }
  s1 = wave_sum(s1) / (float)n;
  s2 = wave_sum(s2) / (float)n;
  const float rs = rstd[row];
  for (int i = lane; i < n; i += 64) {
    const float g = dy[(size_t)row * n + i] * w[i];
    dx[(size_t)row * n + i] = rs * (g - s1 - xhat[(size_t)row * n + i] * s2);
  }
}

__global__ __launch_bounds__(256) void ln_bwd_cols_kernel(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                           float* __restrict__ dw, float* __restrict__ db, int rows, int n) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  float a = 0.f, c = 0.f;
  for (int r = 0; r < rows; ++r) {
    const float g = dy[(size_t)r * n + j];
    a += g * xhat[(size_t)r * n + j];
    c += g;
  }
  dw[j] = a;
  db[j] = c;
}

// ---- several noise draws per observation (fv_head_set_flow_draws): head rows are draw-major, r = s B + b.  The conditioning columns [0, n) of cat (pooled |
// state branch) are computed once on rows 0 .. B - 1 and copied to the rows of draws 1 .. S - 1; their gradient is summed back over the draws.
// grid.y = S - 1: m[(1 + y) B + b][c] <- m[b][c] for c < n
__global__ __launch_bounds__(256) void draws_broadcast_kernel(float* __restrict__ m, int ld, int B, int n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * n) return;
  const int b = (int)(i / n), c = (int)(i % n);
  m[((size_t)(1 + blockIdx.y) * B + b) * ld + c] = m[(size_t)b * ld + c];
}
// m[b][c] <- m[b][c] + m[B + b][c] + .. + m[(S - 1) B + b][c] for c < n, in ascending s.  One thread owns one (b, c): it alone reads that column of the S rows
// and writes row b -- no atomics, a fixed order, two runs give the same bits
__global__ __launch_bounds__(256) void draws_fold_kernel(float* __restrict__ m, int ld, int B, int S, int n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * n) return;
  const int b = (int)(i / n), c = (int)(i % n);
  float acc = m[(size_t)b * ld + c];
  for (int s = 1; s < S; ++s) acc += m[((size_t)s * B + b) * ld + c];
  m[(size_t)b * ld + c] = acc;
}
// the (B, K) pad bytes once per draw: dst[s B K + i] <- src[i]
__global__ __launch_bounds__(256) void draws_pad_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long n, int S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t v = src[i];
  for (int s = 0; s < S; ++s) dst[(size_t)s * n + i] = v;
}
// prefix mode (fv_head_set_flow_prefix): the mask the chunked loss reads, dst[r K + k] = 1 where pad[(r % B) K + k] is set (pad may be null), else 2 where the
// row's prefix mask m[r K + k] is set (conditioned on, not trained, still a valid step), else 0.  n = R K bytes, nobs = B K
__global__ __launch_bounds__(256) void prefix_loss_mask_kernel(const uint8_t* __restrict__ pad, const uint8_t* __restrict__ m, uint8_t* __restrict__ dst, long n,
                                                                long nobs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dst[i] = pad && pad[i % nobs] != 0 ? 1 : (m[i] != 0 ? 2 : 0);
}
// inference on a prefix-width head: the mask columns of cat are 0 (no step is conditioned on)
__global__ __launch_bounds__(256) void zero_cols_kernel(float* __restrict__ dst, int ldd, int B, int N) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * N) return;
  dst[(size_t)(i / N) * ldd + (i % N)] = 0.f;
}

}  // namespace

HeadOffsets head_offsets(const HeadDims& d) {
  HeadOffsets r;
  const int64_t sz[HP_TOTAL] = {d.ds, d.ds, (int64_t)d.hid * d.ds, d.hid, (int64_t)d.fus * head_cat_width(d), d.fus,
                          d.fus, d.fus, (int64_t)d.fus * d.fus, d.fus, (int64_t)head_out_width(d) * d.fus, head_out_width(d)};
  int64_t o = 0;
  for (int i = 0; i < HP_TOTAL; ++i) {
    r.o[i] = o;
    o += (sz[i] + 3) / 4 * 4;  // keep every tensor 16-byte aligned inside the flat buffer
  }
  r.o[HP_TOTAL] = o;
  return r;
}

namespace {
struct Saved {
  float *n0, *xh0, *rstd0, *z1, *cat, *z2, *xh2, *rstd2, *n2, *d2, *mask, *z3, *a3;
  uint8_t* pmask;   // prefix mode: (R, pk) bytes behind everything else (pk == 0: nothing, every offset and the total as ever)
  float* logits;    // bins mode: (R, da, nb) behind that (nb == 0: nothing)
  size_t cat_off, total;   // cat's offset from the base and the whole block, in floats
};
// B observations; the state branch keeps B rows, cat .. a3 have R = head_rows(d, B) of them (more than B only with fv_head_set_flow_draws)
Saved carve(const HeadDims& d, int B, float* base) {
  Saved s;
  size_t o = 0;
  const size_t R = (size_t)head_rows(d, B);
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += (n + 3) / 4 * 4; return p; };
  s.n0 = take((size_t)B * d.ds); s.xh0 = take((size_t)B * d.ds); s.rstd0 = take(B);
  s.z1 = take((size_t)B * d.hid); s.cat_off = o; s.cat = take(R * head_cat_width(d)); s.z2 = take(R * d.fus);
  s.xh2 = take(R * d.fus); s.rstd2 = take(R); s.n2 = take(R * d.fus); s.d2 = take(R * d.fus);
  s.mask = take(R * d.fus); s.z3 = take(R * d.fus); s.a3 = take(R * d.fus);
  s.pmask = reinterpret_cast<uint8_t*>(take(d.te > 0 ? (R * d.pk + 3) / 4 : 0));
  s.logits = take(d.nb > 0 ? R * d.da * d.nb : 0);
  s.total = o;
  return s;
}
}  // namespace

size_t head_saved_bytes(const HeadDims& d, int B) { return carve(d, B, nullptr).total * sizeof(float); }
float* head_saved_cat(const HeadDims& d, int B, float* saved) { return carve(d, B, saved).cat; }
size_t head_saved_cat_offset(const HeadDims& d, int B) { return carve(d, B, nullptr).cat_off; }
uint8_t* head_saved_prefix_mask(const HeadDims& d, int B, float* saved) { return carve(d, B, saved).pmask; }
float* head_saved_logits(const HeadDims& d, int B, float* saved) { return carve(d, B, saved).logits; }

size_t head_bwd_scratch_bytes(const HeadDims& d, int B) {
  const size_t wmax = (size_t)(head_cat_width(d) > d.fus ? head_cat_width(d) : d.fus);
  // dL/dactions | two activation-gradient rows of the widest layer | alignment slack | the chunked loss's per-block partials (loss, sum w d^2, sum w)
  // (draws: every row count is R = S B, and the pad mask's R K <= R da bytes, once per draw, come last; prefix mode builds its loss mask in the same place)
  // (bins mode: dL/dlogits is nb times wider, and the bins loss's per-block partials follow the chunked loss's)
  const size_t R = (size_t)head_rows(d, B);
  return (R * head_out_width(d) + 2 * R * wmax + 64 + chunk_loss_partial_floats() + (d.nb > 0 ? bins_loss_partial_floats((long)(R * d.da)) : 0) + (R > (size_t)B || (d.te > 0 && d.pk > 0) ? (R * d.da + 3) / 4 : 0)) * sizeof(float);
}

void launch_head_state_branch(const HeadDims& d, const float* P, const float* states, int B, float* n0, float* xh0, float* rstd0, float* z1, float* dst, int ldd,
                              hipStream_t s, const HeadIoNorm* io) {
  const HeadOffsets ho = head_offsets(d);
  const dim3 blk(256);
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(cdiv(B, 4)), blk, 0, s, states, d.ds, P + ho.o[HP_STATE_LN_W], P + ho.o[HP_STATE_LN_B], n0, xh0, rstd0, B, d.ds,
                     io ? io->state_mean : nullptr, io ? io->state_istd : nullptr);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.hid, 4), cdiv(B, 8)), blk, 0, s, n0, d.ds, P + ho.o[HP_STATE_W], P + ho.o[HP_STATE_B], dst, ldd, z1, B, d.hid, d.ds, 1,
                     (const float*)nullptr, (const float*)nullptr);
}

int launch_head_forward(const HeadDims& d, const float* P, const float* pooled, const float* states, int B,
                        int training, float drop_p, uint64_t seed, uint64_t offset, float* actions, float* saved,
                        hipStream_t s, const HeadIoNorm* io) {
  if (!P || !pooled || !states || !actions || !saved) return fv_fail(FV_ERR_ARG, "head_forward: null pointer");
  if (d.nb > 0 && (!d.bn || d.te > 0)) return fv_fail(FV_ERR_STATE, "head_forward: bins mode needs its configuration and excludes flow mode");
  if (B <= 0) return fv_fail(FV_ERR_ARG, "head_forward: B must be positive");
  if (drop_p < 0.f || drop_p >= 1.f) return fv_fail(FV_ERR_ARG, "head_forward: dropout p out of range");
  const HeadOffsets ho = head_offsets(d);
  const Saved sv = carve(d, B, saved);
  const int cw = head_cat_width(d);   // flow mode: the x_t and phi(t) columns behind the conditioning part (launch_flow_prepare writes them)
  const dim3 blk(256);
  // the action un-normalisation belongs to inference only: training computes its loss against NORMALISED targets
  const float* as = io && !training ? io->action_std : nullptr;
  const float* am = io && !training ? io->action_mean : nullptr;
  // draws (fv_head_set_flow_draws, training forms only): the state branch and the pooled copy run once per observation, their columns are copied to the rows of
  // draws 1 .. S - 1 and everything from fusion.0 on runs on R = S B head rows (every row its own dropout mask: the element index).  R == B: the launches as ever
  const int R = training ? head_rows(d, B) : B;
  const bool zero_mask = !training && d.te > 0 && d.pk > 0;   // prefix-width head at inference: the mask columns are 0 (a training form reads launch_flow_prepare's)
  training &= 1;   // bit 0: dropout active; any non-zero value: actions stay in normalised space
  // cat = [ pooled | state branch ]: two writers of disjoint columns
  hipLaunchKernelGGL(copy_cols_kernel, dim3(cdiv((long)B * d.feat, 256)), blk, 0, s, pooled, d.feat, sv.cat, cw, B, d.feat);
  launch_head_state_branch(d, P, states, B, sv.n0, sv.xh0, sv.rstd0, sv.z1, sv.cat + d.feat, cw, s, io);
  if (zero_mask) hipLaunchKernelGGL(zero_cols_kernel, dim3(cdiv((long)B * d.pk, 256)), blk, 0, s, sv.cat + (cw - d.pk), cw, B, d.pk);
  if (R > B) hipLaunchKernelGGL(draws_broadcast_kernel, dim3(cdiv((long)B * (d.feat + d.hid), 256), R / B - 1), blk, 0, s, sv.cat, cw, B, d.feat + d.hid);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.fus, 4), cdiv(R, 8)), blk, 0, s, sv.cat, cw, P + ho.o[HP_FUS0_W], P + ho.o[HP_FUS0_B], sv.z2, d.fus, (float*)nullptr, R, d.fus, cw, 0, (const float*)nullptr, (const float*)nullptr);
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(cdiv(R, 4)), blk, 0, s, sv.z2, d.fus, P + ho.o[HP_FUS_LN_W], P + ho.o[HP_FUS_LN_B], sv.n2, sv.xh2, sv.rstd2, R, d.fus,
                     (const float*)nullptr, (const float*)nullptr);
  hipLaunchKernelGGL(silu_dropout_kernel, dim3(cdiv((long)R * d.fus, 256)), blk, 0, s, sv.n2, sv.d2, sv.mask, (long)R * d.fus, training, drop_p, seed, offset);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.fus, 4), cdiv(R, 8)), blk, 0, s, sv.d2, d.fus, P + ho.o[HP_FUS4_W], P + ho.o[HP_FUS4_B], sv.a3, d.fus, sv.z3, R, d.fus, d.fus, 1, (const float*)nullptr, (const float*)nullptr);
  if (d.nb > 0) {   // bins mode: the logits stay in `saved`, `actions` receives the decoded chunk (the action statistics behind the decode)
    const int ow = head_out_width(d);
    hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(ow, 4), cdiv(R, 8)), blk, 0, s, sv.a3, d.fus, P + ho.o[HP_ACT_W], P + ho.o[HP_ACT_B], sv.logits, ow, (float*)nullptr, R, ow, d.fus, 0,
                       (const float*)nullptr, (const float*)nullptr);
    FV_HIP_CHECK(hipGetLastError());
    return launch_bins_decode(*d.bn, sv.logits, actions, nullptr, (long)R * d.da, d.nb, d.da, as, am, s);
  }
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.da, 4), cdiv(R, 8)), blk, 0, s, sv.a3, d.fus, P + ho.o[HP_ACT_W], P + ho.o[HP_ACT_B], actions, d.da, (float*)nullptr, R, d.da, d.fus, 0, as, am);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_head_backward(const HeadDims& d, const float* P, const float* grad_actions, const float* actions,
                         const float* targets, int B, float drop_p, const float* saved, float* loss, float* G,
                         float* scratch, hipStream_t s, float* d_pooled, float loss_scale, const HeadLoss* hl, const float* ga_scale_dev) {
  if (!P || !saved || !G || !scratch) return fv_fail(FV_ERR_ARG, "head_backward: null pointer");
  const bool weighted = hl && hl->dim_w && hl->step_w;   // fv_head_set_loss_weights: every kind takes the chunked kernel's weighted instance
  const bool prefix = d.te > 0 && d.pk > 0;   // fv_head_set_flow_prefix: the conditioned steps are masked out of the loss, so the fused loss is always the chunked kernel
  if (prefix && !grad_actions && (!hl || hl->chunk != d.pk))
    return fv_fail(FV_ERR_STATE, "head_backward: prefix mode needs the loss's chunk length (fv_head_set_loss) to be the prefix's, %d", d.pk);
  const bool chunked = hl && !grad_actions && (hl->kind != FV_LOSS_MSE || hl->pad || weighted || prefix);   // MSE without a mask or weights: mse_kernel, for any chunk length
  if (chunked && (!hl->metrics || hl->chunk < 1 || d.da % hl->chunk)) return fv_fail(FV_ERR_ARG, "head_backward: chunked loss needs metrics and a chunk length that divides action_dim");
  const bool bins = d.nb > 0;
  if (bins) {   // the head's own loss from the saved logits; `actions` is not read
    if (!d.bn || d.te > 0) return fv_fail(FV_ERR_STATE, "head_backward: bins mode needs its configuration and excludes flow mode");
    if (grad_actions) return fv_fail(FV_ERR_STATE, "head_backward: a bins head trains through its own loss (the decode is not differentiated): no grad_actions");
    if (!targets || !loss || !hl || !hl->metrics) return fv_fail(FV_ERR_ARG, "head_backward: the bins loss needs targets, loss and the metrics slot");
    if (hl->kind != FV_LOSS_MSE) return fv_fail(FV_ERR_STATE, "head_backward: the loss kind %d has no meaning for a bins head (cross-entropy): leave it at FV_LOSS_MSE", hl->kind);
    if (hl->chunk < 1 || d.da % hl->chunk) return fv_fail(FV_ERR_ARG, "head_backward: the chunk length must divide action_dim");
  } else if (!grad_actions && (!actions || !targets || !loss)) return fv_fail(FV_ERR_ARG, "head_backward: need grad_actions or (actions, targets, loss)");
  if (B <= 0) return fv_fail(FV_ERR_ARG, "head_backward: B must be positive");
  (void)drop_p;  // the multiplier keep/(1-p) is stored in saved.mask
  const HeadOffsets ho = head_offsets(d);
  const Saved sv = carve(d, B, const_cast<float*>(saved));
  const int cw = head_cat_width(d);   // flow mode: the x_t and phi(t) columns behind the conditioning part (launch_flow_prepare writes them)
  const size_t wmax = (size_t)(cw > d.fus ? cw : d.fus);
  // draws (fv_head_set_flow_draws): B counts observations, the layers down to dcat run on R = S B head rows (actions, targets = u and grad_actions have R rows,
  // the loss divides by all R da elements), then the conditioning columns of dcat are summed over the draws and the state branch runs on B rows.  R == B: as ever
  const int obs = B, S = head_rows(d, B) / B;
  B *= S;
  float* ga_own = scratch;
  const int ow = head_out_width(d);   // rows of action_head.weight: da, or da nb logits in bins mode
  float* g1 = ga_own + ((size_t)B * ow + 3) / 4 * 4;
  float* g2 = g1 + (size_t)B * wmax;
  const dim3 blk(256);
  const unsigned b8 = cdiv(B, 8);
  const float* ga = grad_actions;
  if (bins) {
    float* part = g2 + (size_t)B * wmax + 16;   // (where the chunked loss's partials go; head_bwd_scratch_bytes holds the bins loss's behind them)
    const int rc = launch_bins_loss(*d.bn, sv.logits, targets, hl->pad, ga_own, part, loss, hl->metrics, (long)B * d.da, d.nb, d.da, hl->chunk, loss_scale, s,
                                    weighted ? hl->dim_w : nullptr, weighted ? hl->step_w : nullptr);
    if (rc != FV_OK) return rc;
    ga = ga_own;
  } else if (!ga && chunked) {
    float* part = g2 + (size_t)B * wmax + 16;   // behind everything the layers below use; the 64 floats of slack cover the rounding of B * da and this gap (head_bwd_scratch_bytes)
    const uint8_t* pad = hl->pad;
    if (prefix) {   // pad[r % obs] | m[r], built where the draws' copy of the mask goes
      uint8_t* rep = reinterpret_cast<uint8_t*>(part + chunk_loss_partial_floats());
      const long nk = (long)obs * hl->chunk;
      hipLaunchKernelGGL(prefix_loss_mask_kernel, dim3(cdiv(nk * S, 256)), blk, 0, s, pad, sv.pmask, rep, nk * S, nk);
      pad = rep;
    } else if (S > 1 && pad) {   // the mask is (obs, K): every draw of an observation reads its row, from a copy per draw behind the partials
      uint8_t* rep = reinterpret_cast<uint8_t*>(part + chunk_loss_partial_floats());
      const long nk = (long)obs * hl->chunk;
      hipLaunchKernelGGL(draws_pad_kernel, dim3(cdiv(nk, 256)), blk, 0, s, pad, rep, nk, S);
      pad = rep;
    }
    const int rc = launch_chunk_loss(actions, targets, pad, ga_own, part, loss, hl->metrics, (long)B * d.da, d.da / hl->chunk, hl->kind, hl->beta, loss_scale, s,
                                     weighted ? hl->dim_w : nullptr, weighted ? hl->step_w : nullptr, hl->chunk, prefix);
    if (rc != FV_OK) return rc;
    ga = ga_own;
  } else if (!ga) {
    hipLaunchKernelGGL(mse_kernel, dim3(1), blk, 0, s, actions, targets, loss, ga_own, B * d.da, loss_scale);
    ga = ga_own;
  }
  // the step guard's dynamic factor on top of loss_scale: dL/dactions *= *ga_scale_dev, a power of two read on the device (the gap up to g1 is scratch)
  if (ga_scale_dev && ga == ga_own) {
    const int rc = launch_axpy(ga_own, nullptr, (int64_t)(g1 - ga_own), ga_scale_dev, s);
    if (rc != FV_OK) return rc;
  }
  // action_head
  hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(cdiv(d.fus, 256), ow), blk, 0, s, ga, sv.a3, d.fus, G + ho.o[HP_ACT_W], B, ow, d.fus);
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(ow, 256)), blk, 0, s, ga, G + ho.o[HP_ACT_B], B, ow);
  hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(cdiv(d.fus, 32), b8), blk, 0, s, ga, P + ho.o[HP_ACT_W], g1, d.fus, B, ow, d.fus);
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv((long)B * d.fus, 256)), blk, 0, s, g1, d.fus, sv.z3, (const float*)nullptr, g1, B, d.fus);
  // fusion.4
  hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(cdiv(d.fus, 256), d.fus), blk, 0, s, g1, sv.d2, d.fus, G + ho.o[HP_FUS4_W], B, d.fus, d.fus);
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(d.fus, 256)), blk, 0, s, g1, G + ho.o[HP_FUS4_B], B, d.fus);
  hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(cdiv(d.fus, 32), b8), blk, 0, s, g1, P + ho.o[HP_FUS4_W], g2, d.fus, B, d.fus, d.fus);
  // dropout multiplier, SiLU, LayerNorm (fusion.1)
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv((long)B * d.fus, 256)), blk, 0, s, g2, d.fus, sv.n2, sv.mask, g2, B, d.fus);
  hipLaunchKernelGGL(ln_bwd_cols_kernel, dim3(cdiv(d.fus, 256)), blk, 0, s, g2, sv.xh2, G + ho.o[HP_FUS_LN_W], G + ho.o[HP_FUS_LN_B], B, d.fus);
  hipLaunchKernelGGL(ln_bwd_rows_kernel, dim3(cdiv(B, 4)), blk, 0, s, g2, P + ho.o[HP_FUS_LN_W], sv.xh2, sv.rstd2, g1, B, d.fus);
  // fusion.0
  hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(cdiv(cw, 256), d.fus), blk, 0, s, g1, sv.cat, cw, G + ho.o[HP_FUS0_W], B, d.fus, cw);
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(d.fus, 256)), blk, 0, s, g1, G + ho.o[HP_FUS0_B], B, d.fus);
  hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(cdiv(cw, 32), b8), blk, 0, s, g1, P + ho.o[HP_FUS0_W], g2, cw, B, d.fus, cw);
  if (S > 1) {   // sum the conditioning columns of dcat over the draws into rows 0 .. obs - 1; from here on B counts observations again
    hipLaunchKernelGGL(draws_fold_kernel, dim3(cdiv((long)obs * (d.feat + d.hid), 256)), blk, 0, s, g2, cw, obs, S, d.feat + d.hid);
    B = obs;
  }
  const unsigned o8 = cdiv(B, 8);
  // dcat = [d pooled | d state branch]: the first `feat` columns are what an unfrozen backbone's backward starts from
  if (d_pooled) hipLaunchKernelGGL(copy_cols_kernel, dim3(cdiv((long)B * d.feat, 256)), blk, 0, s, g2, cw, d_pooled, d.feat, B, d.feat);
  // state branch: ds = dcat[:, feat:], SiLU, Linear, LayerNorm
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv((long)B * d.hid, 256)), blk, 0, s, g2 + d.feat, cw, sv.z1, (const float*)nullptr, g1, B, d.hid);
  hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(cdiv(d.ds, 256), d.hid), blk, 0, s, g1, sv.n0, d.ds, G + ho.o[HP_STATE_W], B, d.hid, d.ds);
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(d.hid, 256)), blk, 0, s, g1, G + ho.o[HP_STATE_B], B, d.hid);
  hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(cdiv(d.ds, 32), o8), blk, 0, s, g1, P + ho.o[HP_STATE_W], g2, d.ds, B, d.hid, d.ds);
  hipLaunchKernelGGL(ln_bwd_cols_kernel, dim3(cdiv(d.ds, 256)), blk, 0, s, g2, sv.xh0, G + ho.o[HP_STATE_LN_W], G + ho.o[HP_STATE_LN_B], B, d.ds);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

}  // namespace fv
