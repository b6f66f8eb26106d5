// chunk_kernels.hip -- what an action CHUNK adds around the head (head_kernels.hip), all fp32, every sum in a fixed order (no float atomics):
//   chunk_loss_kernel<WEIGHTED> + its fold   pad-masked L1 / smooth-L1 / MSE over (B, K, A), optionally weighted per dimension and step
//                                            (fv_head_set_loss / _mask / _weights; launch_head_backward runs it when HeadLoss asks for it)
//   loss_per_dim_kernel                      mean |a - t| per action dimension (fv_head_loss_per_dim)
//   loss_per_time_kernel                     the flow head's squared velocity error and element count per time bucket (fv_head_loss_per_time)
//   ensemble_step_kernel                     the temporal-ensembling ring (fv_ensemble_step)
#include "kernels.h"

namespace fv {
namespace {

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
// PREFIX (fv_head_set_flow_prefix): the mask byte is 0 live, 1 padded, 2 masked by the action prefix alone.  Both are selected away; a byte of 2 still counts
// as a valid step, so the valid fraction stays the pad-only one.  The instances without it keep their own expressions: they are the code they were
__device__ __forceinline__ bool chunk_step_live(const uint8_t* __restrict__ pad, long st, unsigned& cnt) {
  if (!pad) return true;
  const uint8_t pb = pad[st];
  cnt += pb == 2;
  return pb == 0;
}
template <bool WEIGHTED, bool PREFIX>
__global__ __launch_bounds__(256) void chunk_loss_kernel(const float* __restrict__ a, const float* __restrict__ t, const uint8_t* __restrict__ pad,
                                                          float* __restrict__ g, float* __restrict__ partial, long n, int A, int kind, float beta,
                                                          float loss_scale, int vec, const float* __restrict__ dim_w, const float* __restrict__ step_w, int K) {
  __shared__ float red[3][4];
  const float nf = (float)n, c = loss_scale / nf;
  float sl = 0.f, sq = 0.f;
  unsigned cnt = 0;
  auto weighted = [&](long i, float ai, float ti) -> float {   // element i of the weighted instance -> g
    const long st = i / A;
    if constexpr (PREFIX) {
      if (!chunk_step_live(pad, st, cnt)) return 0.f;
    } else {
      if (pad && pad[st] != 0) return 0.f;
    }
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
      bool w;
      if constexpr (PREFIX) w = chunk_step_live(pad, i / A, cnt);
      else w = !pad || pad[i / A] == 0;
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
          bool w;
          if constexpr (PREFIX) w = chunk_step_live(pad, (i * 4 + j) / A, cnt);
          else w = !pad || pad[(i * 4 + j) / A] == 0;
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

// block = one time bucket (fv_head_loss_per_time): out[j] = { sum of (a - u)^2, count } over the non-padded elements of the rows whose t falls into bucket j.
// Every block walks the rows in ascending order (t[r] is one uniform load), a thread sums its elements of the bucket's rows in that order, then a fixed-order
// fold (no atomics).  A thread counts its elements in an integer; the fold of the counts is exact in fp32 below 2^24 elements per bucket
__global__ __launch_bounds__(256) void loss_per_time_kernel(const float* __restrict__ a, const float* __restrict__ u, const float* __restrict__ t,
                                                             const uint8_t* __restrict__ pad, float* __restrict__ out, int R, int B, int da, int K, int nb) {
  __shared__ float red[2][4];
  const int j = blockIdx.x, A = da / K;
  float sq = 0.f;
  unsigned cnt = 0;
  for (int r = 0; r < R; ++r) {
    const float tc = fminf(fmaxf(t[r], 0.f), 1.f);
    if (min(nb - 1, (int)(tc * (float)nb)) != j) continue;
    const uint8_t* pr = pad ? pad + (size_t)(r % B) * K : nullptr;   // (the draws of a flow head share their observation's mask)
    for (int i = threadIdx.x; i < da; i += 256) {
      if (pr && pr[i / A] != 0) continue;
      const float d = a[(size_t)r * da + i] - u[(size_t)r * da + i];
      sq += d * d;
      ++cnt;
    }
  }
  sq = wave_sum(sq);
  const float sc = wave_sum((float)cnt);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sq; red[1][threadIdx.x >> 6] = sc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[2 * j] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[2 * j + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
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

}  // namespace

size_t chunk_loss_partial_floats() { return 3 * (size_t)CHUNK_LOSS_BLOCKS; }

int launch_chunk_loss(const float* a, const float* t, const uint8_t* pad, float* g, float* partial, float* loss, float* metrics, long n, int A, int kind,
                      float beta, float loss_scale, hipStream_t s, const float* dim_w, const float* step_w, int K, int prefix) {
  if (!a || !t || !g || !partial || !loss || !metrics) return fv_fail(FV_ERR_ARG, "chunk_loss: null pointer");
  if (n <= 0 || A <= 0 || n % A) return fv_fail(FV_ERR_ARG, "chunk_loss: n must be a positive multiple of the step width");
  if (kind != FV_LOSS_MSE && kind != FV_LOSS_L1 && kind != FV_LOSS_SMOOTH_L1) return fv_fail(FV_ERR_ARG, "chunk_loss: unknown loss kind %d", kind);
  if (kind == FV_LOSS_SMOOTH_L1 && !(beta > 0.f)) return fv_fail(FV_ERR_ARG, "chunk_loss: smooth-L1 beta must be positive");
  const int vec = (((uintptr_t)a | (uintptr_t)t | (uintptr_t)g) & 15) == 0;
  const unsigned want = cdiv(vec ? (n >> 2) : n, 256);
  const unsigned nb = want < 1 ? 1 : (want < (unsigned)CHUNK_LOSS_BLOCKS ? want : (unsigned)CHUNK_LOSS_BLOCKS);
  if (dim_w || step_w) {
    if (!dim_w || !step_w || K < 1 || (n / A) % K) return fv_fail(FV_ERR_ARG, "chunk_loss: weights need both vectors and a chunk length that divides the step count");
    if (prefix) hipLaunchKernelGGL((chunk_loss_kernel<true, true>), dim3(nb), dim3(256), 0, s, a, t, pad, g, partial, n, A, kind, beta, loss_scale, vec, dim_w, step_w, K);
    else hipLaunchKernelGGL((chunk_loss_kernel<true, false>), dim3(nb), dim3(256), 0, s, a, t, pad, g, partial, n, A, kind, beta, loss_scale, vec, dim_w, step_w, K);
  } else if (prefix) {
    hipLaunchKernelGGL((chunk_loss_kernel<false, true>), dim3(nb), dim3(256), 0, s, a, t, pad, g, partial, n, A, kind, beta, loss_scale, vec, (const float*)nullptr,
                       (const float*)nullptr, 1);
  } else {
    hipLaunchKernelGGL((chunk_loss_kernel<false, false>), dim3(nb), dim3(256), 0, s, a, t, pad, g, partial, n, A, kind, beta, loss_scale, vec, (const float*)nullptr,
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

int launch_loss_per_time(const float* a, const float* u, const float* t, const uint8_t* pad, float* out, int R, int B, int da, int K, int nb, hipStream_t s) {
  if (!a || !u || !t || !out) return fv_fail(FV_ERR_ARG, "loss_per_time: null pointer");
  if (B < 1 || R < B || R % B || K < 1 || da < 1 || da % K) return fv_fail(FV_ERR_ARG, "loss_per_time: bad shape");
  if (nb < 1 || nb > FV_LOSS_TIME_BUCKETS_MAX) return fv_fail(FV_ERR_ARG, "loss_per_time: n_buckets = %d outside 1 .. %d", nb, FV_LOSS_TIME_BUCKETS_MAX);
  hipLaunchKernelGGL(loss_per_time_kernel, dim3(nb), dim3(256), 0, s, a, u, t, pad, out, R, B, da, K, nb);
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

}  // namespace fv
