// bins_kernels.hip -- the binned action head (fv_head_set_bins): every action element is a classification over nb uniform bins of its range [lo, hi], all fp32,
// every sum in a fixed order (no float atomics):
//   bins_loss_kernel<SOFT, WEIGHTED> + its fold   log-softmax, cross-entropy against a one-hot or Gaussian-smoothed (HL-Gauss) target, and dL/dlogits, over
//                                                 (B K A) groups of nb logits (launch_head_backward runs it when the head is in bins mode)
//   bins_decode_kernel<MODE>                      logits -> the centre of the most likely bin, or the mean of the centres under softmax(logits)
// ONE WAVE OWNS ONE GROUP.  A lane keeps its at most 16 logits in registers from one read, in one of two bin-to-lane mappings chosen by nb alone:
//   quads  (nb % 256 == 0): register 4 i + c holds bin 4 (lane + 64 i) + c -- one 16-byte load per i when the pointer is aligned, four 4-byte loads otherwise;
//   stride (any other nb):  register i holds bin lane + 64 i.
// The arithmetic and the order of every sum depend on the mapping only, never on the alignment: a misaligned call gives the aligned call's bits.
#include "kernels.h"

namespace fv {
namespace {

constexpr int BINS_REGS = FV_HEAD_BINS_MAX / 64;   // 16

struct BinsGroup {
  float z[BINS_REGS];   // the lane's logits; -inf past the end of the group
  int nreg;             // registers in use: cdiv(nb, 64)
  bool quads;
};
__device__ __forceinline__ int bins_index(const BinsGroup& gr, int r, int lane) { return gr.quads ? 4 * (lane + 64 * (r >> 2)) + (r & 3) : lane + 64 * r; }

__device__ __forceinline__ void bins_load(BinsGroup& gr, const float* __restrict__ zg, int nb, int lane, bool vec) {
  gr.quads = (nb & 255) == 0;
  gr.nreg = (nb + 63) >> 6;
#pragma unroll
  for (int r = 0; r < BINS_REGS; ++r) gr.z[r] = -INFINITY;
  if (gr.quads && vec) {
#pragma unroll
    for (int i = 0; i < BINS_REGS / 4; ++i)
      if (i * 256 < nb) {
        const float4 v = reinterpret_cast<const float4*>(zg)[lane + 64 * i];
        gr.z[4 * i] = v.x; gr.z[4 * i + 1] = v.y; gr.z[4 * i + 2] = v.z; gr.z[4 * i + 3] = v.w;
      }
  } else {
#pragma unroll
    for (int r = 0; r < BINS_REGS; ++r) {
      const int j = bins_index(gr, r, lane);
      if (r < gr.nreg && j < nb) gr.z[r] = zg[j];
    }
  }
}
// v[r] of every live register -> out[bin]; the store form follows the load form
__device__ __forceinline__ void bins_store(const BinsGroup& gr, const float (&v)[BINS_REGS], float* __restrict__ out, int nb, int lane, bool vec) {
  if (gr.quads && vec) {
#pragma unroll
    for (int i = 0; i < BINS_REGS / 4; ++i)
      if (i * 256 < nb) reinterpret_cast<float4*>(out)[lane + 64 * i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else {
#pragma unroll
    for (int r = 0; r < BINS_REGS; ++r) {
      const int j = bins_index(gr, r, lane);
      if (r < gr.nreg && j < nb) out[j] = v[r];
    }
  }
}

// softmax of the group: e[r] = exp(z[r] - max) (0 past the end), their sum, and the lowest index among the largest logits
struct BinsSoftmax { float e[BINS_REGS]; float zmax, sum; int arg; };
__device__ __forceinline__ BinsSoftmax bins_softmax(const BinsGroup& gr, int nb, int lane) {
  BinsSoftmax sm;
  float m = -INFINITY;
  int arg = nb;
#pragma unroll
  for (int r = 0; r < BINS_REGS; ++r) {   // registers in ascending order; within the lane a later register wins only when strictly larger or equal with a lower bin
    const int j = bins_index(gr, r, lane);
    if (r < gr.nreg && j < nb && (gr.z[r] > m || (gr.z[r] == m && j < arg))) { m = gr.z[r]; arg = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (om > m || (om == m && oa < arg)) { m = om; arg = oa; }
  }
  sm.zmax = m; sm.arg = arg;
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < BINS_REGS; ++r) {
    sm.e[r] = r < gr.nreg ? expf(gr.z[r] - m) : 0.f;   // (exp(-inf) = 0 for the lanes past the end)
    s += sm.e[r];
  }
  sm.sum = wave_sum(s);
  return sm;
}

__device__ __forceinline__ float bins_centre(int j, float lo, float w) { return fmaf((float)j + 0.5f, w, lo); }
// sum_j p_j c_j of the group
__device__ __forceinline__ float bins_mean(const BinsGroup& gr, const BinsSoftmax& sm, int nb, int lane, float lo, float w) {
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < BINS_REGS; ++r) {
    const int j = bins_index(gr, r, lane);
    if (r < gr.nreg && j < nb) acc += (sm.e[r] / sm.sum) * bins_centre(j, lo, w);
  }
  return wave_sum(acc);
}

// Phi(x2) - Phi(x1) for x1 <= x2 in double, through erfc on the side where both tails are small (the difference keeps its relative accuracy)
__device__ __forceinline__ double phi_diff(double x1, double x2) {
  const double s = 0.70710678118654752440;
  return x1 > 0.0 ? 0.5 * (erfc(x1 * s) - erfc(x2 * s)) : 0.5 * (erfc(-x2 * s) - erfc(-x1 * s));
}

// ---- the loss.  logits, g: (n, nb); targets (n) continuous, normalised; pad (n / A) bytes or null; range = [lo | hi | w], n_range floats each, element e of a
// row (da = K A of them) reads entry e % n_range.  With p = softmax(z), q the target distribution, om = dim_w[a] step_w[k] (1 when not WEIGHTED):
//   loss = sum_valid om (-sum_j q_j log p_j) / n      g_j = loss_scale om (p_j - q_j) / n
//   metrics = { sum_valid (decoded - target)^2 / n, valid / n, hits / valid, 0 }   (never weighted; valid looks at pads only; an om == 0 element adds nothing
//   to the squared error and is no hit)
// A padded or om == 0 group is SELECTED away: its target is never read, its nb gradient elements are written as 0.
// Every block writes four partials; bins_loss_fold_kernel sums them in ascending order.
template <bool SOFT, bool WEIGHTED>
__global__ __launch_bounds__(256) void bins_loss_kernel(const float* __restrict__ logits, const float* __restrict__ targets, const uint8_t* __restrict__ pad,
                                                         float* __restrict__ g, float* __restrict__ partial, long n, int nb, int da, int A, int K,
                                                         const float* __restrict__ range, int n_range, float sigma, int decode, float loss_scale, int vec,
                                                         const float* __restrict__ dim_w, const float* __restrict__ step_w) {
  __shared__ float red[4][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long grp = (long)blockIdx.x * 4 + wv;
  float out4[4] = {0.f, 0.f, 0.f, 0.f};   // loss, squared error, valid, hit
  if (grp < n) {
    const int e = (int)(grp % da);
    const long step = grp / A;
    const bool valid = !pad || pad[step] == 0;
    float om = 1.f;
    if constexpr (WEIGHTED) om = dim_w[e % A] * step_w[(e / A) % K];
    float gv[BINS_REGS];
#pragma unroll
    for (int r = 0; r < BINS_REGS; ++r) gv[r] = 0.f;
    BinsGroup gr;
    bins_load(gr, logits + grp * nb, nb, lane, vec != 0);
    if (valid) out4[2] = 1.f;
    if (valid && om != 0.f) {
      const BinsSoftmax sm = bins_softmax(gr, nb, lane);
      const float lo = range[e % n_range], hi = range[n_range + e % n_range], w = range[2 * n_range + e % n_range];
      const float t = targets[grp];
      const float a = fminf(fmaxf(t, lo), hi);
      const int idx = min(nb - 1, (int)floorf((a - lo) / w));
      const float lsum = logf(sm.sum), c = loss_scale / (float)n;
      float q[BINS_REGS];
      if constexpr (SOFT) {
        const double dlo = (double)lo, dw = (double)w, dhi = (double)hi, da64 = (double)a, sd = (double)sigma * dw;
        const double Z = phi_diff((dlo - da64) / sd, (dhi - da64) / sd);
        auto edge = [&](int j) { return j >= nb ? dhi : dlo + (double)j * dw; };   // (the last edge is hi itself: sum q = 1 whatever w's rounding)
#pragma unroll
        for (int r = 0; r < BINS_REGS; ++r) {
          const int j = bins_index(gr, r, lane);
          q[r] = r < gr.nreg && j < nb ? (float)(phi_diff((edge(j) - da64) / sd, (edge(j + 1) - da64) / sd) / Z) : 0.f;
        }
      } else {
#pragma unroll
        for (int r = 0; r < BINS_REGS; ++r) q[r] = bins_index(gr, r, lane) == idx ? 1.f : 0.f;
      }
      float ce = 0.f;
#pragma unroll
      for (int r = 0; r < BINS_REGS; ++r) {
        const int j = bins_index(gr, r, lane);
        if (r < gr.nreg && j < nb) {
          if (q[r] != 0.f) ce -= q[r] * ((gr.z[r] - sm.zmax) - lsum);   // (q == 0 is selected away: a logit of -inf next to it gives no 0 * inf)
          gv[r] = c * om * (sm.e[r] / sm.sum - q[r]);
        }
      }
      out4[0] = om * wave_sum(ce);
      const float dec = decode == FV_BINS_DECODE_MEAN ? bins_mean(gr, sm, nb, lane, lo, w) : bins_centre(sm.arg, lo, w);
      const float d = dec - t;
      out4[1] = d * d;
      out4[3] = sm.arg == idx ? 1.f : 0.f;
    }
    bins_store(gr, gv, g + grp * nb, nb, lane, vec != 0);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) red[i][wv] = out4[i];
  }
  __syncthreads();
  if (threadIdx.x < 4) partial[4 * (long)blockIdx.x + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// single block: thread t sums the partials of blocks t, t + 256, ... in ascending order, then a fixed-order fold
__global__ __launch_bounds__(256) void bins_loss_fold_kernel(const float* __restrict__ partial, long nblk, float* __restrict__ loss, float* __restrict__ metrics, long n) {
  __shared__ float red[4][4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (long i = threadIdx.x; i < nblk; i += 256) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += partial[4 * i + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s[j] = wave_sum(s[j]);
    if ((threadIdx.x & 63) == 0) red[j][threadIdx.x >> 6] = s[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (red[j][0] + red[j][1]) + (red[j][2] + red[j][3]);
    *loss = v[0] / (float)n;
    metrics[0] = v[1] / (float)n;
    metrics[1] = v[2] / (float)n;
    metrics[2] = v[2] > 0.f ? v[3] / v[2] : 0.f;
    metrics[3] = 0.f;
  }
}

// ---- decode.  logits (n, nb) -> actions (n, or null when only the probabilities are wanted): MODE 0 the centre of the most likely bin (ties to the lowest index), 1 sum_j p_j c_j; then the folded action
// statistics, actions * post_scale[e] + post_shift[e] (may be null).  probs (n, nb) or null: softmax(logits) as well
template <int MODE>
__global__ __launch_bounds__(256) void bins_decode_kernel(const float* __restrict__ logits, float* __restrict__ actions, float* __restrict__ probs, long n, int nb,
                                                           int da, const float* __restrict__ range, int n_range, int vec, const float* __restrict__ post_scale,
                                                           const float* __restrict__ post_shift) {
  const int lane = threadIdx.x & 63;
  const long grp = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (grp >= n) return;
  const int e = (int)(grp % da);
  BinsGroup gr;
  bins_load(gr, logits + grp * nb, nb, lane, vec != 0);
  const BinsSoftmax sm = bins_softmax(gr, nb, lane);
  const float lo = range[e % n_range], w = range[2 * n_range + e % n_range];
  float v = MODE == FV_BINS_DECODE_MEAN ? bins_mean(gr, sm, nb, lane, lo, w) : bins_centre(sm.arg, lo, w);
  if (post_scale) v = v * post_scale[e] + post_shift[e];
  if (lane == 0 && actions) actions[grp] = v;
  if (probs) {
    float p[BINS_REGS];
#pragma unroll
    for (int r = 0; r < BINS_REGS; ++r) p[r] = sm.e[r] / sm.sum;
    bins_store(gr, p, probs + grp * nb, nb, lane, vec != 0);
  }
}

int bins_check(const char* who, const HeadBins& hb, long n, int nb, int da) {
  if (!hb.range) return fv_fail(FV_ERR_ARG, "%s: null range table", who);
  if (nb < 2 || nb > FV_HEAD_BINS_MAX) return fv_fail(FV_ERR_ARG, "%s: bins = %d outside 2 .. %d", who, nb, FV_HEAD_BINS_MAX);
  if (da < 1 || n < 1 || n % da) return fv_fail(FV_ERR_ARG, "%s: the group count must be a positive multiple of the row's %d elements", who, da);
  if (hb.n_range < 1 || da % hb.n_range) return fv_fail(FV_ERR_ARG, "%s: n_range = %d must divide the row's %d elements", who, hb.n_range, da);
  if (hb.decode != FV_BINS_DECODE_ARGMAX && hb.decode != FV_BINS_DECODE_MEAN) return fv_fail(FV_ERR_ARG, "%s: unknown decode %d", who, hb.decode);
  if (!(hb.sigma >= 0.f) || !std::isfinite(hb.sigma)) return fv_fail(FV_ERR_ARG, "%s: sigma must be finite and >= 0", who);
  if (n > 4L * 0x7fffffff) return fv_fail(FV_ERR_ARG, "%s: too many groups", who);
  return FV_OK;
}

}  // namespace

size_t bins_loss_partial_floats(long n) { return 4 * (size_t)cdiv(n, 4); }

int launch_bins_loss(const HeadBins& hb, const float* logits, const float* targets, const uint8_t* pad, float* g, float* partial, float* loss, float* metrics, long n,
                     int nb, int da, int K, float loss_scale, hipStream_t s, const float* dim_w, const float* step_w) {
  if (!logits || !targets || !g || !partial || !loss || !metrics) return fv_fail(FV_ERR_ARG, "bins_loss: null pointer");
  if (const int rc = bins_check("bins_loss", hb, n, nb, da); rc != FV_OK) return rc;
  if (K < 1 || da % K) return fv_fail(FV_ERR_ARG, "bins_loss: the chunk length %d must divide the row's %d elements", K, da);
  if (!dim_w != !step_w) return fv_fail(FV_ERR_ARG, "bins_loss: weights need both vectors");
  const int A = da / K;
  const int vec = (((uintptr_t)logits | (uintptr_t)g) & 15) == 0;
  const dim3 grid(cdiv(n, 4)), blk(256);
  const bool soft = hb.sigma > 0.f;
#define FV_BINS_LOSS(S, W) hipLaunchKernelGGL((bins_loss_kernel<S, W>), grid, blk, 0, s, logits, targets, pad, g, partial, n, nb, da, A, K, hb.range, hb.n_range, hb.sigma, hb.decode, loss_scale, vec, dim_w, step_w)
  if (soft && dim_w) FV_BINS_LOSS(true, true);
  else if (soft) FV_BINS_LOSS(true, false);
  else if (dim_w) FV_BINS_LOSS(false, true);
  else FV_BINS_LOSS(false, false);
#undef FV_BINS_LOSS
  hipLaunchKernelGGL(bins_loss_fold_kernel, dim3(1), blk, 0, s, partial, (long)grid.x, loss, metrics, n);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_bins_decode(const HeadBins& hb, const float* logits, float* actions, float* probs, long n, int nb, int da, const float* post_scale, const float* post_shift,
                       hipStream_t s) {
  if (!logits || (!actions && !probs)) return fv_fail(FV_ERR_ARG, "bins_decode: null pointer");
  if (!post_scale != !post_shift) return fv_fail(FV_ERR_ARG, "bins_decode: the action statistics need both vectors");
  if (const int rc = bins_check("bins_decode", hb, n, nb, da); rc != FV_OK) return rc;
  const int vec = (((uintptr_t)logits | (uintptr_t)probs) & 15) == 0;
  const dim3 grid(cdiv(n, 4)), blk(256);
  if (hb.decode == FV_BINS_DECODE_MEAN)
    hipLaunchKernelGGL((bins_decode_kernel<FV_BINS_DECODE_MEAN>), grid, blk, 0, s, logits, actions, probs, n, nb, da, hb.range, hb.n_range, vec, post_scale, post_shift);
  else
    hipLaunchKernelGGL((bins_decode_kernel<FV_BINS_DECODE_ARGMAX>), grid, blk, 0, s, logits, actions, probs, n, nb, da, hb.range, hb.n_range, vec, post_scale, post_shift);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

}  // namespace fv
