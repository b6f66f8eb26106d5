// head_kernels.hip -- the only trainable part of the path, all fp32 (the reference keeps it fp32 too):
//   action expert forward     reference fastvla/fastvlm_with_expert.py:23-38,50-54
//   MSE + hand-derived backward for the 12 head tensors   fastvla/modeling_fastvla.py:56, trainer.py:175
//   fused global-norm clip + AdamW on one flat buffer      trainer.py:60-66,178-180; lerobot configuration_fastvla.py:51-55
// 3.05 M parameters / ~18 MFLOP per sample: launch-latency bound, so the kernels are simple wave-per-output fp32
// dot products with coalesced weight reads; parameters and gradients are views into flat caller-owned buffers.
#include "kernels.h"

namespace fv {
namespace {

constexpr float LN_EPS = 1e-5f;

// ---- Philox4x32-10 (counter-based; (seed, offset) explicit so a step is reproducible) ----
__device__ __forceinline__ uint4 philox(uint4 c, uint2 k) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u; k.y += 0xBB67AE85u;
  }
  return c;
}

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

// ---- chunked action loss (fv_head_set_loss / fv_head_set_loss_mask) ----
// a, t: (B, K, A) row-major, n = B K A elements; pad (may be null): (B, K) bytes, 1 = the step lies past the episode end.  With w = !pad and d = a - t:
//   loss = sum w rho(d) / n      g = loss_scale w rho'(d) / n      metrics = { sum w d^2 / n, sum w / n }   (the denominator is ALL n elements: LeRobot's
//   `(loss * ~pad).mean()`, which keeps gradient accumulation and the data-parallel mean exact when micro-batches hold different pad counts)
// A padded element is SELECTED away, never multiplied: whatever its target holds (NaN, +-inf) it gives 0 to the loss, the metrics and g.
// Many blocks; every block writes three partials in a fixed order and chunk_loss_fold_kernel sums them in a fixed order (no float atomics: two runs
// and two replicas agree bit for bit).  vec: a, t, g are 16-byte aligned -> float4 body, the n % 4 tail goes through the scalar form in block 0.
constexpr int CHUNK_LOSS_BLOCKS = 256;
struct LossTerm { float rho, grad; };
__device__ __forceinline__ LossTerm loss_term(float d, int kind, float beta, float c, float loss_scale, float nf) {
  const float ad = fabsf(d), sg = d > 0.f ? c : (d < 0.f ? -c : 0.f);   // c = loss_scale / n
  if (kind == FV_LOSS_L1) return {ad, sg};
  if (kind == FV_LOSS_SMOOTH_L1) return ad < beta ? LossTerm{0.5f * d * d / beta, loss_scale * (d / beta) / nf} : LossTerm{ad - 0.5f * beta, sg};
  return {d * d, loss_scale * 2.0f * d / nf};   // mse_kernel's expression
}
// s + round(d * d), never fma(d, d, s): the unweighted instance's own sequence for the masked MSE (its d * d feeds rho too and is not contracted into the sum),
// which the weighted instance has to repeat for all-ones weights to give the same bits
__device__ __forceinline__ float add_square_rounded(float s, float d) {
#pragma clang fp contract(off)
  const float dd = d * d;
  return s + dd;
}
// WEIGHTED (fv_head_set_loss_weights): om = dim_w[i % A] * step_w[(i / A) % K] scales rho and g; an element with om == 0 is selected away like a padded
// one (0 to the loss, to g and to the masked MSE, whatever its target holds).  The two metrics stay unweighted and the valid count looks at pads only.
// om == 1 changes no bit: x * 1.0f is exact, and a contracted fma(rho, 1, s) is s + rho.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void chunk_loss_kernel(const float* __restrict__ a, const float* __restrict__ t, const uint8_t* __restrict__ pad,
                                                          float* __restrict__ g, float* __restrict__ partial, long n, int A, int kind, float beta,
                                                          float loss_scale, int vec, const float* __restrict__ dim_w, const float* __restrict__ step_w, int K) {
  __shared__ float red[3][4];
  const float nf = (float)n, c = loss_scale / nf;
  float sl = 0.f, sq = 0.f;
  unsigned cnt = 0;
  auto weighted = [&](long i, float ai, float ti) -> float {   // element i of the weighted instance -> g
    const long st = i / A;
    if (pad && pad[st] != 0) return 0.f;
    ++cnt;
    const float om = dim_w[i - st * A] * step_w[st % K];
    if (om == 0.f) return 0.f;
    const float d = ai - ti;
    const LossTerm r = loss_term(d, kind, beta, c, loss_scale, nf);
    sl += om * r.rho;
    sq = add_square_rounded(sq, d);
    return om * r.grad;
  };
  auto one = [&](long i) {
    if constexpr (WEIGHTED) {
      g[i] = weighted(i, a[i], t[i]);
    } else {
      const bool w = !pad || pad[i / A] == 0;
      LossTerm r{0.f, 0.f};
      if (w) {
        const float d = a[i] - t[i];
        r = loss_term(d, kind, beta, c, loss_scale, nf);
        sl += r.rho; sq += d * d; ++cnt;
      }
      g[i] = r.grad;
    }
  };
  if (vec) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
      const float4 av = reinterpret_cast<const float4*>(a)[i], tv = reinterpret_cast<const float4*>(t)[i];
      const float ae[4] = {av.x, av.y, av.z, av.w}, te[4] = {tv.x, tv.y, tv.z, tv.w};
      float ge[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (WEIGHTED) {
          ge[j] = weighted(i * 4 + j, ae[j], te[j]);
        } else {
          const bool w = !pad || pad[(i * 4 + j) / A] == 0;
          LossTerm r{0.f, 0.f};
          if (w) {
            const float d = ae[j] - te[j];
            r = loss_term(d, kind, beta, c, loss_scale, nf);
            sl += r.rho; sq += d * d; ++cnt;
          }
          ge[j] = r.grad;
        }
      }
      reinterpret_cast<float4*>(g)[i] = make_float4(ge[0], ge[1], ge[2], ge[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) one((n4 << 2) + threadIdx.x);
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) one(i);
  }
  sl = wave_sum(sl); sq = wave_sum(sq);
  const float sc = wave_sum((float)cnt);   // a thread sees at most n / 256 + 4 elements: exact in fp32 for every n below 2^24
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sl; red[1][threadIdx.x >> 6] = sq; red[2][threadIdx.x >> 6] = sc; }
  __syncthreads();
  if (threadIdx.x < 3) partial[3 * blockIdx.x + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}
// single block: loss = sum of the blocks' loss partials / n, metrics = { sum w d^2 / n, sum w / n }
__global__ __launch_bounds__(256) void chunk_loss_fold_kernel(const float* __restrict__ partial, int nb, float* __restrict__ loss,
                                                               float* __restrict__ metrics, long n) {
  __shared__ float red[3][4];
  float s[3] = {0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < nb; i += 256) { s[0] += partial[3 * i]; s[1] += partial[3 * i + 1]; s[2] += partial[3 * i + 2]; }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    s[j] = wave_sum(s[j]);
    if ((threadIdx.x & 63) == 0) red[j][threadIdx.x >> 6] = s[j];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const float v = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3])) / (float)n;
    if (threadIdx.x == 0) *loss = v; else metrics[threadIdx.x - 1] = v;
  }
}

// block = one action dimension: out[j] = mean |a - t| over the non-padded rows (steps) of column j, 0 when there is none.  Every thread sums its rows in
// order, then a fixed-order fold (no float atomics); a thread counts at most rows / 256 + 1 steps, exact in fp32 below 2^24 rows per thread
__global__ __launch_bounds__(256) void loss_per_dim_kernel(const float* __restrict__ a, const float* __restrict__ t, const uint8_t* __restrict__ pad,
                                                            float* __restrict__ out, long rows, int A, long pad_rows) {
  __shared__ float red[2][4];
  const int j = blockIdx.x;
  float sa = 0.f;
  unsigned cnt = 0;
  for (long r = threadIdx.x; r < rows; r += 256) {
    if (pad && pad[r % pad_rows] != 0) continue;   // pad_rows < rows: the flow head's draws (fv_head_set_flow_draws) share their observation's mask
    sa += fabsf(a[r * A + j] - t[r * A + j]);
    ++cnt;
  }
  sa = wave_sum(sa);
  const float sc = wave_sum((float)cnt);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sa; red[1][threadIdx.x >> 6] = sc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), m = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    out[j] = m > 0.f ? s / m : 0.f;
  }
}

// ---- temporal ensembling of action chunks (fv_ensemble_step; LeRobot's ACTTemporalEnsembler, per environment) ----
// Ring: slot (head + k) % K holds the running average for the time step k ahead of now; row k of the new chunk is one more prediction of it.  A slot with
// count n == 0 takes the row as it is, otherwise ens <- (ens cw[n-1] + c w[n]) / cw[n] with w[i] = exp(-coeff i) (i = 0 the oldest) and cw its running sum.
// The head slot (k == 0) goes to `actions` and its count returns to 0: it is the slot of time now + K on the next call.
// ONE THREAD OWNS ONE (env, slot): it reads the slot's count once, loops over the slot's A elements and rewrites the count itself -- no other thread reads
// or writes that word or those elements, so there is no barrier, no atomic and no reduction, and two runs agree bit for bit.
__global__ __launch_bounds__(256) void ensemble_step_kernel(const float* __restrict__ chunks, float* __restrict__ ens, int32_t* __restrict__ count,
                                                             float* __restrict__ actions, const float* __restrict__ w, const float* __restrict__ cw,
                                                             long slots, int K, int A, int head) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // env * K + slot
  if (idx >= slots) return;
  const long env = idx / K;
  const int slot = (int)(idx - env * K);
  const int k = slot >= head ? slot - head : slot - head + K;
  int n = count[idx];
  n = n < 0 ? 0 : (n > K - 1 ? K - 1 : n);   // (a slot sees K predictions at the most: n <= K - 1 here; the clamp keeps the table reads in bounds whatever the state holds)
  const float* c = chunks + (env * K + k) * A;
  float* e = ens + idx * A;
  float* o = k == 0 ? actions + env * A : e;
  if (n == 0) {
    for (int j = 0; j < A; ++j) o[j] = c[j];
  } else {
    const float wn = w[n], c0 = cw[n - 1], c1 = cw[n];
    for (int j = 0; j < A; ++j) o[j] = (e[j] * c0 + c[j] * wn) / c1;
  }
  count[idx] = k == 0 ? 0 : (n + 1 < K ? n + 1 : K);
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

// ---- AdamW + clip ----
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
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ v, long n,
                                                     fv_adamw_hparams hp, float bc1, float bc2_sqrt,
                                                     const float* __restrict__ sumsq, float* __restrict__ norm_out,
                                                     float* __restrict__ e, float ema_w) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  // torch clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max = 1)
  const float norm = sqrtf(*sumsq) * hp.grad_scale;
  float coef = hp.grad_scale;
  if (hp.max_grad_norm > 0.f) coef *= fminf(hp.max_grad_norm / (norm + 1e-6f), 1.0f);
  if (i == 0 && norm_out) *norm_out = norm;
  if (i >= n) return;
  float pi = p[i], mi = m[i], vi = v[i];
  adamw_update(pi, g[i], mi, vi, coef, hp.lr, hp.weight_decay, hp.beta1, hp.beta2, hp.eps, bc1, bc2_sqrt);   // (shared with adamw_groups_kernel: common.h)
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
  if constexpr (EMA) e[i] = ema_update(e[i], pi, ema_w);
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

// block = one head row, grid (B, S): head row r = s B + b is draw s of observation b (fv_head_set_flow_draws; S == 1: the rows as ever).  It reads targets[b]
// and draws what row b draws at offset + (s << 56) -- the key, the counter (group, b, offset) and the Box-Muller as they are, so row b's draws depend
// neither on B nor on S, and draw 0 is the single draw.  Explicit noise (S B, da) / tin (S B) are read at r.
// cat: the row-major (S B, cw) matrix inside `saved`; columns [xo, xo + da) <- x_t, [xo + da, xo + da + te) <- phi(t); u_out (S B, da) <- eps - a.
// x_t is formed in double and rounded once: t eps and (1 - t) a cancel for some rows, and the fp32 form then loses bits the loss target does not
__global__ __launch_bounds__(256) void flow_prepare_kernel(const float* __restrict__ targets, const float* __restrict__ noise, const float* __restrict__ tin,
                                                            float* __restrict__ cat, int cw, int xo, float* __restrict__ u_out, int da, int te,
                                                            const float* __restrict__ freq, int time_dist, float dist_a, float dist_b, uint64_t seed,
                                                            uint64_t offset) {
  const int obs = blockIdx.x, row = blockIdx.y * gridDim.x + obs;
  offset += (uint64_t)blockIdx.y << 56;
  float t;
  if (tin) {
    t = tin[row];
  } else {
    const uint4 r = flow_philox(0u, (uint32_t)obs, seed, offset);
    if (time_dist == 0) t = (float)(r.x >> 8) * FLOW_U24;
    else t = 1.0f / (1.0f + expf(-(dist_a + dist_b * flow_box_muller(r.x, r.y).x)));
  }
  float* xr = cat + (size_t)row * cw + xo;
  const double td = (double)t, omt = 1.0 - td;
  for (int g = threadIdx.x; g * 4 < da; g += 256) {
    float n[4] = {0.f, 0.f, 0.f, 0.f};
    if (!noise) flow_normals4(1u + (uint32_t)g, (uint32_t)obs, seed, offset, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = g * 4 + j;
      if (i >= da) break;
      const float e = noise ? noise[(size_t)row * da + i] : n[j], a = targets[(size_t)obs * da + i];
      xr[i] = (float)(td * (double)e + omt * (double)a);
      u_out[(size_t)row * da + i] = e - a;
    }
  }
  for (int i = threadIdx.x; i < te / 2; i += 256) flow_phi(xr + da, freq, te / 2, t, i);
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

// the sampler's start: xphi (B, da + te) <- [ noise or the draws of (seed, offset) | phi(t0) ]
__global__ __launch_bounds__(256) void flow_init_kernel(const float* __restrict__ noise, float* __restrict__ xphi, int da, int te, const float* __restrict__ freq,
                                                         float t0, uint64_t seed, uint64_t offset) {
  const int row = blockIdx.x;
  float* xr = xphi + (size_t)row * (da + te);
  for (int g = threadIdx.x; g * 4 < da; g += 256) {
    float n[4] = {0.f, 0.f, 0.f, 0.f};
    if (!noise) flow_normals4(1u + (uint32_t)g, (uint32_t)row, seed, offset, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = g * 4 + j;
      if (i >= da) break;
      xr[i] = noise ? noise[(size_t)row * da + i] : n[j];
    }
  }
  for (int i = threadIdx.x; i < te / 2; i += 256) flow_phi(xr + da, freq, te / 2, t0, i);
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
__global__ __launch_bounds__(256) void flow_cond_kernel(const float* __restrict__ pooled, int feat, const float* __restrict__ sb, int hid, const float* __restrict__ W,
                                                         int ldw, const float* __restrict__ bias, float* __restrict__ c, int B, int N) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), b0 = blockIdx.y * 8;
  if (n >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  flow_dot8(pooled, feat, W + (size_t)n * ldw, feat, b0, B, lane, acc);
  flow_dot8(sb, hid, W + (size_t)n * ldw + feat, hid, b0, B, lane, acc);
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
// step kernel C: v = ba[n] + Wa[n] . a3[b]; x <- x + dt v in the epilogue (the lane that owns (b, n) reads and writes x[b][n], nobody else touches it).
// Not the last step: the blocks of column group 0 also write phi(t_next) for their 8 rows.  The last step writes `actions`, with the folded action statistics
__global__ __launch_bounds__(256) void flow_step_c_kernel(const float* __restrict__ a3, int K, const float* __restrict__ W, const float* __restrict__ bias,
                                                           float* __restrict__ xphi, int xw, int te, float dt, float t_next, const float* __restrict__ freq,
                                                           float* __restrict__ actions, const float* __restrict__ post_scale, const float* __restrict__ post_shift,
                                                           int B, int N) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), b0 = blockIdx.y * 8;
  if (!actions && blockIdx.x == 0) {
    const int half = te / 2;
    for (int idx = threadIdx.x; idx < 8 * half; idx += 256) {
      const int j = idx / half, i = idx - j * half;
      if (b0 + j < B) flow_phi(xphi + (size_t)(b0 + j) * xw + N, freq, half, t_next, i);
    }
  }
  if (n >= N) return;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  flow_dot8(a3, K, W + (size_t)n * K, K, b0, B, lane, acc);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0)
    for (int j = 0; j < 8 && b0 + j < B; ++j) {
      const size_t b = (size_t)(b0 + j);
      const float xn = xphi[b * xw + n] + dt * (acc[j] + bias[n]);
      if (!actions) xphi[b * xw + n] = xn;
      else actions[b * N + n] = post_scale ? xn * post_scale[n] + post_shift[n] : xn;
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
// x + dt v as ONE fused multiply-add, the contraction flow_step_c_kernel's `x + dt * v` compiles to: with v' == v the guided update repeats its bits.
// (the same for the folded action statistics x scale + shift)
__device__ __forceinline__ float flow_fma_pinned(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// The last kernel of a guided step, one thread per (b, n): J^T omega = sum_q part[q][b][n] (the fusion.0 product's partials), g = omega - t J^T omega,
// v' = v - k g, x <- x + dt v'; phi(t_next), or on the last step `actions` (with the folded statistics) and chunk_out (without), as flow_step_c_kernel.
// jt_out != null (the op-level entry): J^T omega alone
__global__ __launch_bounds__(256) void flow_guide_update_kernel(const float* __restrict__ part, int S_in, const float* __restrict__ omega, const float* __restrict__ v,
                                                                 float* __restrict__ xphi, int xw, int te, float t, float kw, float dt, float t_next,
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
  const float xn = flow_fma_pinned(dt, vp, xphi[(size_t)b * xw + n]);
  if (!actions) { xphi[(size_t)b * xw + n] = xn; return; }
  if (chunk_out) chunk_out[e] = xn;
  actions[e] = post_scale ? flow_fma_pinned(xn, post_scale[n], post_shift[n]) : xn;
}

inline unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

HeadOffsets head_offsets(const HeadDims& d) {
  HeadOffsets r;
  const int64_t sz[12] = {d.ds, d.ds, (int64_t)d.hid * d.ds, d.hid, (int64_t)d.fus * head_cat_width(d), d.fus,
                          d.fus, d.fus, (int64_t)d.fus * d.fus, d.fus, (int64_t)d.da * d.fus, d.da};
  int64_t o = 0;
  for (int i = 0; i < 12; ++i) {
    r.o[i] = o;
    o += (sz[i] + 3) / 4 * 4;  // keep every tensor 16-byte aligned inside the flat buffer
  }
  r.o[12] = o;
  return r;
}

namespace {
struct Saved {
  float *n0, *xh0, *rstd0, *z1, *cat, *z2, *xh2, *rstd2, *n2, *d2, *mask, *z3, *a3;
  size_t total;
};
// B observations; the state branch keeps B rows, cat .. a3 have R = head_rows(d, B) of them (more than B only with fv_head_set_flow_draws)
Saved carve(const HeadDims& d, int B, float* base) {
  Saved s;
  size_t o = 0;
  const size_t R = (size_t)head_rows(d, B);
  auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += (n + 3) / 4 * 4; return p; };
  s.n0 = take((size_t)B * d.ds); s.xh0 = take((size_t)B * d.ds); s.rstd0 = take(B);
  s.z1 = take((size_t)B * d.hid); s.cat = take(R * head_cat_width(d)); s.z2 = take(R * d.fus);
  s.xh2 = take(R * d.fus); s.rstd2 = take(R); s.n2 = take(R * d.fus); s.d2 = take(R * d.fus);
  s.mask = take(R * d.fus); s.z3 = take(R * d.fus); s.a3 = take(R * d.fus);
  s.total = o;
  return s;
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

size_t head_saved_bytes(const HeadDims& d, int B) { return carve(d, B, nullptr).total * sizeof(float); }

size_t head_bwd_scratch_bytes(const HeadDims& d, int B) {
  const size_t wmax = (size_t)(head_cat_width(d) > d.fus ? head_cat_width(d) : d.fus);
  // dL/dactions | two activation-gradient rows of the widest layer | alignment slack | the chunked loss's per-block partials (loss, sum w d^2, sum w)
  // (draws: every row count is R = S B, and the pad mask's R K <= R da bytes, once per draw, come last)
  const size_t R = (size_t)head_rows(d, B);
  return (R * d.da + 2 * R * wmax + 64 + 3 * (size_t)CHUNK_LOSS_BLOCKS + (R > (size_t)B ? (R * d.da + 3) / 4 : 0)) * sizeof(float);
}

int launch_head_forward(const HeadDims& d, const float* P, const float* pooled, const float* states, int B,
                        int training, float drop_p, uint64_t seed, uint64_t offset, float* actions, float* saved,
                        hipStream_t s, const HeadIoNorm* io) {
  if (!P || !pooled || !states || !actions || !saved) return fv_fail(FV_ERR_ARG, "head_forward: null pointer");
  if (B <= 0) return fv_fail(FV_ERR_ARG, "head_forward: B must be positive");
  if (drop_p < 0.f || drop_p >= 1.f) return fv_fail(FV_ERR_ARG, "head_forward: dropout p out of range");
  const HeadOffsets ho = head_offsets(d);
  const Saved sv = carve(d, B, saved);
  const int cw = head_cat_width(d);   // flow mode: the x_t and phi(t) columns behind the conditioning part (launch_flow_prepare writes them)
  const dim3 blk(256);
  const float* sm = io ? io->state_mean : nullptr;
  const float* si = io ? io->state_istd : nullptr;
  // the action un-normalisation belongs to inference only: training computes its loss against NORMALISED targets
  const float* as = io && !training ? io->action_std : nullptr;
  const float* am = io && !training ? io->action_mean : nullptr;
  // draws (fv_head_set_flow_draws, training forms only): the state branch and the pooled copy run once per observation, their columns are copied to the rows of
  // draws 1 .. S - 1 and everything from fusion.0 on runs on R = S B head rows (every row its own dropout mask: the element index).  R == B: the launches as ever
  const int R = training ? head_rows(d, B) : B;
  training &= 1;   // bit 0: dropout active; any non-zero value: actions stay in normalised space
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(cdiv(B, 4)), blk, 0, s, states, d.ds, P + ho.o[0], P + ho.o[1], sv.n0, sv.xh0, sv.rstd0, B, d.ds, sm, si);
  hipLaunchKernelGGL(copy_cols_kernel, dim3(cdiv((long)B * d.feat, 256)), blk, 0, s, pooled, d.feat, sv.cat, cw, B, d.feat);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.hid, 4), cdiv(B, 8)), blk, 0, s, sv.n0, d.ds, P + ho.o[2], P + ho.o[3], sv.cat + d.feat, cw, sv.z1, B, d.hid, d.ds, 1, (const float*)nullptr, (const float*)nullptr);
  if (R > B) hipLaunchKernelGGL(draws_broadcast_kernel, dim3(cdiv((long)B * (d.feat + d.hid), 256), R / B - 1), blk, 0, s, sv.cat, cw, B, d.feat + d.hid);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.fus, 4), cdiv(R, 8)), blk, 0, s, sv.cat, cw, P + ho.o[4], P + ho.o[5], sv.z2, d.fus, (float*)nullptr, R, d.fus, cw, 0, (const float*)nullptr, (const float*)nullptr);
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(cdiv(R, 4)), blk, 0, s, sv.z2, d.fus, P + ho.o[6], P + ho.o[7], sv.n2, sv.xh2, sv.rstd2, R, d.fus,
                     (const float*)nullptr, (const float*)nullptr);
  hipLaunchKernelGGL(silu_dropout_kernel, dim3(cdiv((long)R * d.fus, 256)), blk, 0, s, sv.n2, sv.d2, sv.mask, (long)R * d.fus, training, drop_p, seed, offset);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.fus, 4), cdiv(R, 8)), blk, 0, s, sv.d2, d.fus, P + ho.o[8], P + ho.o[9], sv.a3, d.fus, sv.z3, R, d.fus, d.fus, 1, (const float*)nullptr, (const float*)nullptr);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.da, 4), cdiv(R, 8)), blk, 0, s, sv.a3, d.fus, P + ho.o[10], P + ho.o[11], actions, d.da, (float*)nullptr, R, d.da, d.fus, 0, as, am);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

size_t chunk_loss_partial_floats() { return 3 * (size_t)CHUNK_LOSS_BLOCKS; }

int launch_chunk_loss(const float* a, const float* t, const uint8_t* pad, float* g, float* partial, float* loss, float* metrics, long n, int A, int kind,
                      float beta, float loss_scale, hipStream_t s, const float* dim_w, const float* step_w, int K) {
  if (!a || !t || !g || !partial || !loss || !metrics) return fv_fail(FV_ERR_ARG, "chunk_loss: null pointer");
  if (n <= 0 || A <= 0 || n % A) return fv_fail(FV_ERR_ARG, "chunk_loss: n must be a positive multiple of the step width");
  if (kind != FV_LOSS_MSE && kind != FV_LOSS_L1 && kind != FV_LOSS_SMOOTH_L1) return fv_fail(FV_ERR_ARG, "chunk_loss: unknown loss kind %d", kind);
  if (kind == FV_LOSS_SMOOTH_L1 && !(beta > 0.f)) return fv_fail(FV_ERR_ARG, "chunk_loss: smooth-L1 beta must be positive");
  const int vec = (((uintptr_t)a | (uintptr_t)t | (uintptr_t)g) & 15) == 0;
  const unsigned want = cdiv(vec ? (n >> 2) : n, 256);
  const unsigned nb = want < 1 ? 1 : (want < (unsigned)CHUNK_LOSS_BLOCKS ? want : (unsigned)CHUNK_LOSS_BLOCKS);
  if (dim_w || step_w) {
    if (!dim_w || !step_w || K < 1 || (n / A) % K) return fv_fail(FV_ERR_ARG, "chunk_loss: weights need both vectors and a chunk length that divides the step count");
    hipLaunchKernelGGL(chunk_loss_kernel<true>, dim3(nb), dim3(256), 0, s, a, t, pad, g, partial, n, A, kind, beta, loss_scale, vec, dim_w, step_w, K);
  } else {
    hipLaunchKernelGGL(chunk_loss_kernel<false>, dim3(nb), dim3(256), 0, s, a, t, pad, g, partial, n, A, kind, beta, loss_scale, vec, (const float*)nullptr,
                       (const float*)nullptr, 1);
  }
  hipLaunchKernelGGL(chunk_loss_fold_kernel, dim3(1), dim3(256), 0, s, partial, (int)nb, loss, metrics, n);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_loss_per_dim(const float* a, const float* t, const uint8_t* pad, float* out, long rows, int A, hipStream_t s, long pad_rows) {
  if (!a || !t || !out) return fv_fail(FV_ERR_ARG, "loss_per_dim: null pointer");
  if (rows <= 0 || A <= 0) return fv_fail(FV_ERR_ARG, "loss_per_dim: rows and the step width must be positive");
  if (pad_rows <= 0) pad_rows = rows;
  if (rows % pad_rows) return fv_fail(FV_ERR_ARG, "loss_per_dim: the mask's rows must divide the rows");
  hipLaunchKernelGGL(loss_per_dim_kernel, dim3(A), dim3(256), 0, s, a, t, pad, out, rows, A, pad_rows);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_ensemble_step(const float* chunks, float* ens, int32_t* count, float* actions, const float* w, const float* cw, int n_env, int K, int A, int head,
                         hipStream_t s) {
  if (!chunks || !ens || !count || !actions || !w || !cw) return fv_fail(FV_ERR_ARG, "ensemble_step: null pointer");
  if (n_env < 1 || K < 1 || A < 1 || head < 0 || head >= K) return fv_fail(FV_ERR_ARG, "ensemble_step: bad shape or ring position");
  const long slots = (long)n_env * K;
  hipLaunchKernelGGL(ensemble_step_kernel, dim3(cdiv(slots, 256)), dim3(256), 0, s, chunks, ens, count, actions, w, cw, slots, K, A, head);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_head_backward(const HeadDims& d, const float* P, const float* grad_actions, const float* actions,
                         const float* targets, int B, float drop_p, const float* saved, float* loss, float* G,
                         float* scratch, hipStream_t s, float* d_pooled, float loss_scale, const HeadLoss* hl) {
  if (!P || !saved || !G || !scratch) return fv_fail(FV_ERR_ARG, "head_backward: null pointer");
  const bool weighted = hl && hl->dim_w && hl->step_w;   // fv_head_set_loss_weights: every kind takes the chunked kernel's weighted instance
  const bool chunked = hl && !grad_actions && (hl->kind != FV_LOSS_MSE || hl->pad || weighted);   // MSE without a mask or weights: mse_kernel, for any chunk length
  if (chunked && (!hl->metrics || hl->chunk < 1 || d.da % hl->chunk)) return fv_fail(FV_ERR_ARG, "head_backward: chunked loss needs metrics and a chunk length that divides action_dim");
  if (!grad_actions && (!actions || !targets || !loss)) return fv_fail(FV_ERR_ARG, "head_backward: need grad_actions or (actions, targets, loss)");
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
  float* g1 = ga_own + ((size_t)B * d.da + 3) / 4 * 4;
  float* g2 = g1 + (size_t)B * wmax;
  const dim3 blk(256);
  const unsigned b8 = cdiv(B, 8);
  const float* ga = grad_actions;
  if (!ga && chunked) {
    float* part = g2 + (size_t)B * wmax + 16;   // behind everything the layers below use; the 64 floats of slack cover the rounding of B * da and this gap (head_bwd_scratch_bytes)
    const uint8_t* pad = hl->pad;
    if (S > 1 && pad) {   // the mask is (obs, K): every draw of an observation reads its row, from a copy per draw behind the partials
      uint8_t* rep = reinterpret_cast<uint8_t*>(part + 3 * (size_t)CHUNK_LOSS_BLOCKS);
      const long nk = (long)obs * hl->chunk;
      hipLaunchKernelGGL(draws_pad_kernel, dim3(cdiv(nk, 256)), blk, 0, s, pad, rep, nk, S);
      pad = rep;
    }
    const int rc = launch_chunk_loss(actions, targets, pad, ga_own, part, loss, hl->metrics, (long)B * d.da, d.da / hl->chunk, hl->kind, hl->beta, loss_scale, s,
                                     weighted ? hl->dim_w : nullptr, weighted ? hl->step_w : nullptr, hl->chunk);
    if (rc != FV_OK) return rc;
    ga = ga_own;
  } else if (!ga) {
    hipLaunchKernelGGL(mse_kernel, dim3(1), blk, 0, s, actions, targets, loss, ga_own, B * d.da, loss_scale);
    ga = ga_own;
  }
  // action_head
  hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(cdiv(d.fus, 256), d.da), blk, 0, s, ga, sv.a3, d.fus, G + ho.o[10], B, d.da, d.fus);
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(d.da, 256)), blk, 0, s, ga, G + ho.o[11], B, d.da);
  hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(cdiv(d.fus, 32), b8), blk, 0, s, ga, P + ho.o[10], g1, d.fus, B, d.da, d.fus);
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv((long)B * d.fus, 256)), blk, 0, s, g1, d.fus, sv.z3, (const float*)nullptr, g1, B, d.fus);
  // fusion.4
  hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(cdiv(d.fus, 256), d.fus), blk, 0, s, g1, sv.d2, d.fus, G + ho.o[8], B, d.fus, d.fus);
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(d.fus, 256)), blk, 0, s, g1, G + ho.o[9], B, d.fus);
  hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(cdiv(d.fus, 32), b8), blk, 0, s, g1, P + ho.o[8], g2, d.fus, B, d.fus, d.fus);
  // dropout multiplier, SiLU, LayerNorm (fusion.1)
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv((long)B * d.fus, 256)), blk, 0, s, g2, d.fus, sv.n2, sv.mask, g2, B, d.fus);
  hipLaunchKernelGGL(ln_bwd_cols_kernel, dim3(cdiv(d.fus, 256)), blk, 0, s, g2, sv.xh2, G + ho.o[6], G + ho.o[7], B, d.fus);
  hipLaunchKernelGGL(ln_bwd_rows_kernel, dim3(cdiv(B, 4)), blk, 0, s, g2, P + ho.o[6], sv.xh2, sv.rstd2, g1, B, d.fus);
  // fusion.0
  hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(cdiv(cw, 256), d.fus), blk, 0, s, g1, sv.cat, cw, G + ho.o[4], B, d.fus, cw);
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(d.fus, 256)), blk, 0, s, g1, G + ho.o[5], B, d.fus);
  hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(cdiv(cw, 32), b8), blk, 0, s, g1, P + ho.o[4], g2, cw, B, d.fus, cw);
  if (S > 1) {   // sum the conditioning columns of dcat over the draws into rows 0 .. obs - 1; from here on B counts observations again
    hipLaunchKernelGGL(draws_fold_kernel, dim3(cdiv((long)obs * (d.feat + d.hid), 256)), blk, 0, s, g2, cw, obs, S, d.feat + d.hid);
    B = obs;
  }
  const unsigned o8 = cdiv(B, 8);
  // dcat = [d pooled | d state branch]: the first `feat` columns are what an unfrozen backbone's backward starts from
  if (d_pooled) hipLaunchKernelGGL(copy_cols_kernel, dim3(cdiv((long)B * d.feat, 256)), blk, 0, s, g2, cw, d_pooled, d.feat, B, d.feat);
  // state branch: ds = dcat[:, feat:], SiLU, Linear, LayerNorm
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv((long)B * d.hid, 256)), blk, 0, s, g2 + d.feat, cw, sv.z1, (const float*)nullptr, g1, B, d.hid);
  hipLaunchKernelGGL(linear_bwd_dw_kernel, dim3(cdiv(d.ds, 256), d.hid), blk, 0, s, g1, sv.n0, d.ds, G + ho.o[2], B, d.hid, d.ds);
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(d.hid, 256)), blk, 0, s, g1, G + ho.o[3], B, d.hid);
  hipLaunchKernelGGL(linear_bwd_dx_kernel, dim3(cdiv(d.ds, 32), o8), blk, 0, s, g1, P + ho.o[2], g2, d.ds, B, d.hid, d.ds);
  hipLaunchKernelGGL(ln_bwd_cols_kernel, dim3(cdiv(d.ds, 256)), blk, 0, s, g2, sv.xh0, G + ho.o[0], G + ho.o[1], B, d.ds);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_flow_prepare(const HeadDims& d, const HeadFlow& f, const float* targets, int B, uint64_t seed, uint64_t offset, const float* noise, const float* t,
                        float* saved, float* u_out, hipStream_t s) {
  if (d.te <= 0 || !f.freq) return fv_fail(FV_ERR_STATE, "flow_prepare: the head is not in flow mode (fv_head_set_flow)");
  if (!targets || !saved || !u_out) return fv_fail(FV_ERR_ARG, "flow_prepare: null pointer");
  if (B <= 0) return fv_fail(FV_ERR_ARG, "flow_prepare: B must be positive");
  const int S = head_rows(d, B) / B;
  if (S > 1 && (offset >> 56 & 15)) return fv_fail(FV_ERR_ARG, "flow_prepare: bits 56 .. 59 of the offset number the draws and must be 0 with more than one draw");
  const Saved sv = carve(d, B, saved);
  hipLaunchKernelGGL(flow_prepare_kernel, dim3(B, S), dim3(256), 0, s, targets, noise, t, sv.cat, head_cat_width(d), d.feat + d.hid, u_out, d.da, d.te, f.freq,
                     f.time_dist, f.dist_a, f.dist_b, seed, offset);
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
}  // namespace

size_t flow_sample_scratch_bytes(const HeadDims& d, int B) { return d.te > 0 ? flow_carve(d, B, nullptr).total * sizeof(float) : 0; }

// 4 launches of conditioning (state LayerNorm, state projection, the t-independent part of fusion.0, the start), then 3 per Euler step.  No dropout, no
// atomics, no host synchronisation; t_i = 1 - i / N and dt = -1 / N are rounded once on the host and travel as kernel arguments
int launch_flow_sample(const HeadDims& d, const HeadFlow& f, const float* P, const float* pooled, const float* states, int B, int n_steps, const float* noise,
                       uint64_t seed, uint64_t offset, float* actions, float* scratch, hipStream_t s, const HeadIoNorm* io) {
  if (d.te <= 0 || !f.freq) return fv_fail(FV_ERR_STATE, "flow_sample: the head is not in flow mode (fv_head_set_flow)");
  if (!P || !pooled || !states || !actions || !scratch) return fv_fail(FV_ERR_ARG, "flow_sample: null pointer");
  if (B <= 0 || n_steps < 1) return fv_fail(FV_ERR_ARG, "flow_sample: B and n_steps must be positive");
  const HeadOffsets ho = head_offsets(d);
  const FlowScratch fs = flow_carve(d, B, scratch);
  const int cw = head_cat_width(d), xo = d.feat + d.hid, xw = d.da + d.te;
  const dim3 blk(256);
  const unsigned b8 = cdiv(B, 8);
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(cdiv(B, 4)), blk, 0, s, states, d.ds, P + ho.o[0], P + ho.o[1], fs.n0, fs.xh0, fs.rstd0, B, d.ds,
                     io ? io->state_mean : nullptr, io ? io->state_istd : nullptr);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.hid, 4), b8), blk, 0, s, fs.n0, d.ds, P + ho.o[2], P + ho.o[3], fs.sb, d.hid, fs.z1, B, d.hid, d.ds, 1,
                     (const float*)nullptr, (const float*)nullptr);
  hipLaunchKernelGGL(flow_cond_kernel, dim3(cdiv(d.fus, 4), b8), blk, 0, s, pooled, d.feat, fs.sb, d.hid, P + ho.o[4], cw, P + ho.o[5], fs.c, B, d.fus);
  hipLaunchKernelGGL(flow_init_kernel, dim3(B), blk, 0, s, noise, fs.xphi, d.da, d.te, f.freq, 1.0f, seed, offset);
  const float dt = (float)(-1.0 / (double)n_steps);
  for (int i = 0; i < n_steps; ++i) {
    const bool last = i + 1 == n_steps;
    const float t_next = (float)(1.0 - (double)(i + 1) / (double)n_steps);
    hipLaunchKernelGGL(flow_step_a_kernel, dim3(cdiv(d.fus, 4), b8), blk, 0, s, fs.xphi, xw, P + ho.o[4], cw, xo, fs.c, fs.z2, B, d.fus);
    hipLaunchKernelGGL(flow_step_b_kernel<false>, dim3(cdiv(d.fus, 4), b8), blk, 0, s, fs.z2, P + ho.o[6], P + ho.o[7], P + ho.o[8], P + ho.o[9], fs.a3,
                       (float*)nullptr, B, d.fus);
    hipLaunchKernelGGL(flow_step_c_kernel, dim3(cdiv(d.da, 4), b8), blk, 0, s, fs.a3, d.fus, P + ho.o[10], P + ho.o[11], fs.xphi, xw, d.te, dt, t_next, f.freq,
                       last ? actions : (float*)nullptr, last && io ? io->action_std : (const float*)nullptr, last && io ? io->action_mean : (const float*)nullptr,
                       B, d.da);
  }
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

namespace {
// the guided sampler's rows: the unguided sampler's, then z3, v, omega, dz2 and two partial-sum buffers the transposed products alternate between
struct GuideScratch { FlowScratch fs; float *z3, *v, *omega, *dz2, *pa, *pb; size_t total; };
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
// the conditioning of a sampler call (4 launches): state LayerNorm, state projection, the t-independent part of fusion.0, the start [x | phi(t0)]
void flow_condition(const HeadDims& d, const HeadFlow& f, const HeadOffsets& ho, const FlowScratch& fs, const float* P, const float* pooled, const float* states,
                    int B, const float* noise, float t0, uint64_t seed, uint64_t offset, hipStream_t s, const HeadIoNorm* io) {
  const dim3 blk(256);
  const unsigned b8 = cdiv(B, 8);
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(cdiv(B, 4)), blk, 0, s, states, d.ds, P + ho.o[0], P + ho.o[1], fs.n0, fs.xh0, fs.rstd0, B, d.ds,
                     io ? io->state_mean : nullptr, io ? io->state_istd : nullptr);
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(cdiv(d.hid, 4), b8), blk, 0, s, fs.n0, d.ds, P + ho.o[2], P + ho.o[3], fs.sb, d.hid, fs.z1, B, d.hid, d.ds, 1,
                     (const float*)nullptr, (const float*)nullptr);
  hipLaunchKernelGGL(flow_cond_kernel, dim3(cdiv(d.fus, 4), b8), blk, 0, s, pooled, d.feat, fs.sb, d.hid, P + ho.o[4], head_cat_width(d), P + ho.o[5], fs.c, B, d.fus);
  hipLaunchKernelGGL(flow_init_kernel, dim3(B), blk, 0, s, noise, fs.xphi, d.da, d.te, f.freq, t0, seed, offset);
}
// forward of a guided step: A, B with z3 kept, C' (v, and omega when step_w is given)
void guide_forward(const HeadDims& d, const HeadOffsets& ho, const GuideScratch& g, const float* P, int B, float t, const float* prev, const float* step_w,
                   const int32_t* row_mask, int chunk, int shift, float* v_out, hipStream_t s) {
  const dim3 blk(256);
  const unsigned b8 = cdiv(B, 8);
  const int xw = d.da + d.te;
  hipLaunchKernelGGL(flow_step_a_kernel, dim3(cdiv(d.fus, 4), b8), blk, 0, s, g.fs.xphi, xw, P + ho.o[4], head_cat_width(d), d.feat + d.hid, g.fs.c, g.fs.z2, B, d.fus);
  hipLaunchKernelGGL(flow_step_b_kernel<true>, dim3(cdiv(d.fus, 4), b8), blk, 0, s, g.fs.z2, P + ho.o[6], P + ho.o[7], P + ho.o[8], P + ho.o[9], g.fs.a3, g.z3, B,
                     d.fus);
  hipLaunchKernelGGL(flow_guide_c_kernel, dim3(cdiv(d.da, 4), b8), blk, 0, s, g.fs.a3, d.fus, P + ho.o[10], P + ho.o[11], g.fs.xphi, xw, t, prev, step_w, row_mask,
                     chunk, d.da / chunk, shift, v_out, g.omega, B, d.da);
}
// J^T omega as partial sums: action_head^T over the first n_live rows (the steps behind them have omega == 0), fusion.4^T, LayerNorm, fusion.0[:, x]^T.
// -> the number of partials (B, da) left in g.pa, which flow_guide_update_kernel folds
int guide_backward(const HeadDims& d, const HeadOffsets& ho, const GuideScratch& g, const float* P, const float* omega, int n_live, int B, hipStream_t s) {
  const dim3 blk(256);
  const unsigned b8 = cdiv(B, 8);
  const int rps = guide_rps(B), sd = (int)cdiv(n_live, rps), sf = (int)cdiv(d.fus, rps);
  hipLaunchKernelGGL(flow_vjp_t_kernel<0>, dim3(cdiv(d.fus, 64), b8, sd), blk, 0, s, omega, d.da, 0, (const float*)nullptr, P + ho.o[10], d.fus, 0, g.pa, B, n_live,
                     d.fus, rps);
  hipLaunchKernelGGL(flow_vjp_t_kernel<1>, dim3(cdiv(d.fus, 64), b8, sf), blk, 0, s, g.pa, d.fus, sd, g.z3, P + ho.o[8], d.fus, 0, g.pb, B, d.fus, d.fus, rps);
  hipLaunchKernelGGL(flow_guide_ln_kernel, dim3(B), dim3(d.fus >= 1024 ? 1024 : 256), 0, s, g.fs.z2, P + ho.o[6], P + ho.o[7], g.pb, sf, g.dz2, B, d.fus);
  hipLaunchKernelGGL(flow_vjp_t_kernel<0>, dim3(cdiv(d.da, 64), b8, sf), blk, 0, s, g.dz2, d.fus, 0, (const float*)nullptr, P + ho.o[4], head_cat_width(d),
                     d.feat + d.hid, g.pa, B, d.fus, d.da, rps);
  return sf;
}
}  // namespace

size_t flow_guided_scratch_bytes(const HeadDims& d, int B) { return d.te > 0 ? guide_carve(d, B, nullptr).total * sizeof(float) : 0; }

// Conditioning as launch_flow_sample, then 8 launches per Euler step: A, B (z3 kept), C' (v and omega), three transposed products with a LayerNorm backward
// between the last two, and the update.  t_i, k_i, dt, shift and the live-row count are host values that travel as kernel arguments
int launch_flow_sample_guided(const HeadDims& d, const HeadFlow& f, const HeadGuide& gd, const float* P, const float* pooled, const float* states, int B, int n_steps,
                              const float* noise, uint64_t seed, uint64_t offset, const float* prev, int shift, const int32_t* row_mask, float* actions,
                              float* chunk_out, float* scratch, hipStream_t s, const HeadIoNorm* io) {
  if (d.te <= 0 || !f.freq) return fv_fail(FV_ERR_STATE, "flow_sample_guided: the head is not in flow mode (fv_head_set_flow)");
  if (!gd.step_w || gd.chunk < 1 || d.da % gd.chunk) return fv_fail(FV_ERR_STATE, "flow_sample_guided: guidance is not configured (fv_head_set_flow_guidance)");
  if (!P || !pooled || !states || !prev || !actions || !scratch) return fv_fail(FV_ERR_ARG, "flow_sample_guided: null pointer");
  if (B <= 0 || n_steps < 1) return fv_fail(FV_ERR_ARG, "flow_sample_guided: B and n_steps must be positive");
  if (shift < 0 || shift > gd.chunk) return fv_fail(FV_ERR_ARG, "flow_sample_guided: shift = %d outside 0 .. chunk = %d", shift, gd.chunk);
  const HeadOffsets ho = head_offsets(d);
  const GuideScratch g = guide_carve(d, B, scratch);
  const int A = d.da / gd.chunk, xw = d.da + d.te;
  // steps from here on have omega == 0 (weight 0, or beyond the shift): the first product stops there.  (At least one step: its omega is then all 0)
  const int n_live = std::max(1, std::min(gd.live_steps, gd.chunk - shift)) * A;
  flow_condition(d, f, ho, g.fs, P, pooled, states, B, noise, 1.0f, seed, offset, s, io);
  const float dt = (float)(-1.0 / (double)n_steps);
  for (int i = 0; i < n_steps; ++i) {
    const bool last = i + 1 == n_steps;
    const float t = (float)(1.0 - (double)i / (double)n_steps), t_next = (float)(1.0 - (double)(i + 1) / (double)n_steps);
    const double td = (double)t;
    // k_i = min(beta, ((1 - t)^2 + t^2) / ((1 - t) t)), beta at t = 1: in double from the fp32-rounded t, rounded once
    const float kw = t >= 1.0f ? gd.beta : (float)std::min((double)gd.beta, ((1.0 - td) * (1.0 - td) + td * td) / ((1.0 - td) * td));
    guide_forward(d, ho, g, P, B, t, prev, gd.step_w, row_mask, gd.chunk, shift, g.v, s);
    const int sp = guide_backward(d, ho, g, P, g.omega, n_live, B, s);
    hipLaunchKernelGGL(flow_guide_update_kernel, dim3(cdiv(d.da, 256), B), dim3(256), 0, s, g.pa, sp, g.omega, g.v, g.fs.xphi, xw, d.te, t, kw, dt, t_next, f.freq,
                       last ? actions : (float*)nullptr, last ? chunk_out : (float*)nullptr, last && io ? io->action_std : (const float*)nullptr,
                       last && io ? io->action_mean : (const float*)nullptr, (float*)nullptr, B, d.da);
  }
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
  hipLaunchKernelGGL(flow_guide_update_kernel, dim3(cdiv(d.da, 256), B), dim3(256), 0, s, g.pa, sp, omega, v_out, g.fs.xphi, d.da + d.te, d.te, t, 0.f, 0.f, 0.f,
                     f.freq, (float*)nullptr, (float*)nullptr, (const float*)nullptr, (const float*)nullptr, jt_out, B, d.da);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_axpy(float* y, const float* x, int64_t n, const float* scale_dev, hipStream_t s) {
  // the flat head buffers keep every tensor 16-byte aligned and their total a multiple of 4 elements (head_offsets)
  if (n % 4 || ((uintptr_t)y & 15) || ((uintptr_t)x & 15)) return fv_fail(FV_ERR_ARG, "axpy: buffers must be 16-byte aligned, n %% 4 == 0");
  const unsigned nb = cdiv(n / 4, 256);
  hipLaunchKernelGGL(axpy_kernel, dim3(nb < 1024 ? nb : 1024), dim3(256), 0, s, y, x, (long)(n / 4), scale_dev);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_adamw_clip(float* p, const float* g, float* m, float* v, int64_t n, const fv_adamw_hparams& hp,
                      int64_t step, float* norm_scratch, float* grad_norm_out, hipStream_t s, float* ema, float ema_weight) {
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
  if (ema && ema_weight != 0.f)   // (weight 0 leaves the average alone: the plain instance, which never reads it)
    hipLaunchKernelGGL(adamw_kernel<true>, dim3(nb), dim3(256), 0, s, p, g, m, v, (long)n, hp, bc1, bc2, (const float*)norm_scratch, grad_norm_out, ema, ema_weight);
  else
    hipLaunchKernelGGL(adamw_kernel<false>, dim3(nb), dim3(256), 0, s, p, g, m, v, (long)n, hp, bc1, bc2, (const float*)norm_scratch, grad_norm_out, (float*)nullptr, 0.f);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

}  // namespace fv
