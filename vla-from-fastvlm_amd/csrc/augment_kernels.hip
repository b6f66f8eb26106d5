// augment_kernels.hip -- on-device image augmentation of the training input pipeline (an extension of this build: the reference has none).
//   augment_draw_kernel        one fv_augment_sample per image: a random crop window and a brightness / contrast / saturation matrix, drawn
//                              with Philox4x32-10 from (seed, offset, global sample index) -- head_kernels.hip's dropout convention
//   augment_letterbox_kernel   letterbox_kernel (tower_kernels.hip) sampling THROUGH the crop window and mapping the colour of every image-region
//                              pixel: crop + resize + letterbox is ONE bilinear sample per output pixel, the jitter one affine map of it
// With an identity row (0, 0, Win, Hin, colour = 0) the store kernel evaluates letterbox_kernel's expressions (letterbox.h) on the same
// values: t + 0.0f is exact, (float)Win / (float)rw is the scale the host computes, and lerp(a, a, w) past the last column is kept.
#include "kernels.h"
#include "letterbox.h"

#include <cmath>

namespace fv {
namespace {

// (Philox4x32-10 itself: common.h philox, the one generator the head's dropout and the flow head's draws use too)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct DrawArgs {
  fv_augment_config cfg;
  const void* img; int dtype, B, C, Hin, Win;
  uint64_t seed, offset, sample_base;
  fv_augment_sample* table;
  int need_mean, colour;
};

// One block per sample.  The channel means (contrast's pivot) come first: u8 sources in exact integer sums, f32 sources in a fixed-order tree of
// doubles (per-thread strided partials -> wave -> LDS -> one thread): no atomics, the same bits for a given shape every time.  Thread 0 then draws
// the sample's two Philox blocks and writes its row.  The few dozen operations of a row run in double and round to fp32 once per field.
__global__ __launch_bounds__(256) void augment_draw_kernel(DrawArgs a) {
  __shared__ double part[3][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nc = a.C >= 3 ? 3 : 1;
  const size_t hw = (size_t)a.Hin * a.Win;
  if (a.need_mean) {
    for (int c = 0; c < nc; ++c) {
      const size_t plane = ((size_t)b * a.C + c) * hw;
      double s;
      if (a.dtype == FV_U8) {
        const uint8_t* src = static_cast<const uint8_t*>(a.img) + plane;
        unsigned long long acc = 0;
        for (size_t i = tid; i < hw; i += 256) acc += src[i];
        s = (double)wave_sum_u64(acc);       // < 2^53: exact
      } else {
        const float* src = static_cast<const float*>(a.img) + plane;
        double acc = 0.0;
        for (size_t i = tid; i < hw; i += 256) acc += (double)src[i];
        s = wave_sum_f64(acc);
      }
      if (lane == 0) part[c][wave] = s;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  double mu = 0.0;
  if (a.need_mean) {
    double m[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < nc; ++c) m[c] = (((part[c][0] + part[c][1]) + part[c][2]) + part[c][3]) / (double)hw;
    mu = nc == 1 ? m[0] : 0.299 * m[0] + 0.587 * m[1] + 0.114 * m[2];
  }
  const uint64_t g = a.sample_base + (uint64_t)b, c0 = 2 * g, c1 = 2 * g + 1;
  const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  const uint32_t olo = (uint32_t)a.offset, ohi = (uint32_t)(a.offset >> 32);
  const uint4 r0 = philox(make_uint4((uint32_t)c0, (uint32_t)(c0 >> 32), olo, ohi), key);
  const uint4 r1 = philox(make_uint4((uint32_t)c1, (uint32_t)(c1 >> 32), olo, ohi), key);
  const uint32_t rv[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
  double u[8];
  for (int k = 0; k < 8; ++k) u[k] = (double)(rv[k] >> 8) * (1.0 / 16777216.0);
  const fv_augment_config& f = a.cfg;
  auto mix = [](double lo, double hi, double t) { return lo + (hi - lo) * t; };
  const double W = (double)a.Win, H = (double)a.Hin;
  const double area = mix(f.crop_area[0], f.crop_area[1], u[0]);
  const double rho = exp(mix(log((double)f.crop_ratio[0]), log((double)f.crop_ratio[1]), u[1]));
  const double cw = fmax(fmin(W * sqrt(area * rho), W), 1.0), ch = fmax(fmin(H * sqrt(area / rho), H), 1.0);
  fv_augment_sample o;
  o.cw = (float)cw; o.ch = (float)ch;
  o.x0 = (float)(u[2] * (W - cw)); o.y0 = (float)(u[3] * (H - ch));
  const double bf = mix(f.brightness[0], f.brightness[1], u[4]), cf = mix(f.contrast[0], f.contrast[1], u[5]);
  const double sf = mix(f.saturation[0], f.saturation[1], u[6]);       // (u[7] is reserved)
  const double w3[3] = {0.299, 0.587, 0.114};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.m[i * 3 + j] = a.colour ? (float)(bf * cf * ((i == j ? sf : 0.0) + (1.0 - sf) * w3[j])) : (i == j ? 1.0f : 0.0f);
    o.o[i] = a.colour ? (float)((1.0 - cf) * bf * mu) : 0.0f;
  }
  o.colour = a.colour;
  o.pad[0] = o.pad[1] = o.pad[2] = 0;
  a.table[b] = o;
}

// letterbox_kernel<0>'s shape: one thread = one output column x LB_R rows, blockIdx.z = the sample, so its 80-byte row is block-uniform (scalar
// loads).  Differences: the source coordinate goes through the window (x0 + the window's own scale), and an image-region pixel's fp32 RGB goes
// through clamp(M v + o, 0, value_max) when the row asks for colour.
__global__ __launch_bounds__(256) void augment_letterbox_kernel(LbParams p, const fv_augment_sample* __restrict__ table, float value_max) {
  const int x = blockIdx.x * 256 + threadIdx.x, yb = blockIdx.y * LB_R, b = blockIdx.z;
  if (x >= p.S) return;
  const fv_augment_sample& a = table[b];
  const float sw = __fdiv_rn(a.cw, (float)p.rw), sh = __fdiv_rn(a.ch, (float)p.rh);
  const float wx0 = a.x0, wy0 = a.y0;
  const int colour = a.colour;
  // src = max((dst + 0.5) * scale - 0.5 + origin, 0): lb_src's expression with the window's origin added BEFORE the max (t + 0.0f is exact).  A NaN
  // is absorbed by the max, +inf samples index 0; the index is clamped on both sides, so no row content reads outside the image.
  auto src = [](int d, float scale, float org) {
#pragma clang fp contract(off)
    const float t = ((float)d + 0.5f) * scale - 0.5f;
    const float s = fmaxf(t + org, 0.0f);
    return s < INFINITY ? s : 0.0f;
  };
  auto idx = [](float s, int n) { return max(0, min((int)fminf(s, 1.0e9f), n - 1)); };
  const int dx = x - p.pl;
  const bool xin = dx >= 0 && dx < p.rw;
  const float sx = src(dx, sw, wx0);
  const int x0 = idx(sx, p.Win), x1 = min(x0 + 1, p.Win - 1);
  const float wx = lb_frac(sx, x0);
  const int nc = p.C >= 3 ? 3 : 1;
  float t0[3] = {0.f, 0.f, 0.f}, t1[3] = {0.f, 0.f, 0.f};   // the two source rows, already blended along x
  int have = -1;
#pragma unroll
  for (int r = 0; r < LB_R; ++r) {
    const int y = yb + r;
    if (y >= p.S) break;
    float v[3] = {p.pad, p.pad, p.pad};
    const int dy = y - p.pt;
    if (xin && dy >= 0 && dy < p.rh) {
      const float sy = src(dy, sh, wy0);
      const int y0 = idx(sy, p.Hin), y1 = min(y0 + 1, p.Hin - 1);
      const float wy = lb_frac(sy, y0);
      if (y0 != have) {
        have = y0;
        for (int c = 0; c < nc; ++c) {
          const size_t plane = ((size_t)b * p.C + c) * p.Hin * p.Win;
          const float p00 = lb_fetch(p, plane, y0, x0), p01 = lb_fetch(p, plane, y0, x1);
          const float p10 = lb_fetch(p, plane, y1, x0), p11 = lb_fetch(p, plane, y1, x1);
          t0[c] = lb_lerp(p00, p01, wx);
          t1[c] = lb_lerp(p10, p11, wx);
        }
      }
      for (int c = 0; c < nc; ++c) v[c] = lb_lerp(t0[c], t1[c], wy);
      if (nc == 1) v[1] = v[2] = v[0];  // gray -> repeat
      if (colour) {
        const float r0 = v[0], g0 = v[1], b0 = v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float t = __builtin_fmaf(a.m[c * 3 + 0], r0, __builtin_fmaf(a.m[c * 3 + 1], g0, __builtin_fmaf(a.m[c * 3 + 2], b0, a.o[c])));
          v[c] = fminf(fmaxf(t, 0.0f), value_max);
        }
      }
    }
    uint2 o;
    o.x = pack_bf2(v[0], v[1]);
    o.y = pack_bf2(v[2], 0.0f);
    *reinterpret_cast<uint2*>(p.pix + (((size_t)b * p.S + y) * p.S + x) * 4) = o;
  }
}

bool range_ok(const float* r, bool positive) {   // lo <= hi, finite, lo >= 0 (positive: lo > 0)
  return std::isfinite(r[0]) && std::isfinite(r[1]) && r[0] <= r[1] && (positive ? r[0] > 0.0f : r[0] >= 0.0f);
}
bool is_one(const float* r) { return r[0] == 1.0f && r[1] == 1.0f; }

}  // namespace

#ifndef FV_TRY_RC
#define FV_TRY_RC(expr) do { const int rc_ = (expr); if (rc_ != FV_OK) return rc_; } while (0)
#endif

int launch_augment_draw(const fv_augment_config* cfg, const void* img, int dtype, int B, int C, int Hin, int Win, uint64_t seed, uint64_t offset,
                        uint64_t sample_base, fv_augment_sample* table, hipStream_t s) {
  if (!cfg || !table) return fv_fail(FV_ERR_ARG, "augment_draw: null pointer");
  if (B <= 0 || Hin <= 0 || Win <= 0) return fv_fail(FV_ERR_ARG, "augment_draw: empty shape");
  if (C != 1 && C != 3 && C != 4) return fv_fail(FV_ERR_ARG, "augment_draw: C must be 1, 3 or 4 (got %d)", C);
  if (dtype != FV_F32 && dtype != FV_U8) return fv_fail(FV_ERR_ARG, "augment_draw: dtype must be f32 or u8");
  if (!range_ok(cfg->crop_area, true)) return fv_fail(FV_ERR_ARG, "augment_draw: crop_area must be 0 < lo <= hi (got %g, %g)", cfg->crop_area[0], cfg->crop_area[1]);
  if (!range_ok(cfg->crop_ratio, true)) return fv_fail(FV_ERR_ARG, "augment_draw: crop_ratio must be 0 < lo <= hi (got %g, %g)", cfg->crop_ratio[0], cfg->crop_ratio[1]);
  if (!range_ok(cfg->brightness, false) || !range_ok(cfg->contrast, false) || !range_ok(cfg->saturation, false))
    return fv_fail(FV_ERR_ARG, "augment_draw: brightness / contrast / saturation must be 0 <= lo <= hi");
  DrawArgs a;
  a.cfg = *cfg;
  a.need_mean = is_one(cfg->contrast) ? 0 : 1;        // the gray mean is contrast's pivot: nothing else reads the image
  a.colour = (is_one(cfg->brightness) && is_one(cfg->contrast) && is_one(cfg->saturation)) ? 0 : 1;
  if (a.need_mean && !img) return fv_fail(FV_ERR_ARG, "augment_draw: a contrast range other than (1, 1) needs the images (img is null)");
  a.img = img; a.dtype = dtype; a.B = B; a.C = C; a.Hin = Hin; a.Win = Win;
  a.seed = seed; a.offset = offset; a.sample_base = sample_base; a.table = table;
  hipLaunchKernelGGL(augment_draw_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_letterbox_augmented(const void* img, int dtype, int B, int C, int Hin, int Win, int S, float pad_value, int letterbox,
                               const fv_augment_sample* table, float value_max, bf16_t* pix, hipStream_t s) {
  if (!img || !pix || !table) return fv_fail(FV_ERR_ARG, "letterbox_augmented: null pointer");
  if (!(value_max > 0.0f) || !std::isfinite(value_max)) return fv_fail(FV_ERR_ARG, "letterbox_augmented: value_max must be positive (got %g)", value_max);
  LbParams p;
  FV_TRY_RC(lb_params(img, dtype, B, C, Hin, Win, S, pad_value, letterbox, pix, p));
  if (B > 65535) return fv_fail(FV_ERR_ARG, "letterbox_augmented: B=%d exceeds the grid's 65535 samples", B);
  hipLaunchKernelGGL(augment_letterbox_kernel, dim3((S + 255) / 256, (S + LB_R - 1) / LB_R, B), dim3(256), 0, s, p, table, value_max);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

}  // namespace fv
