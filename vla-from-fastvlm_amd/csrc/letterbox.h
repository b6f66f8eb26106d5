// letterbox.h -- the letterbox's geometry and sampling expressions, shared by the kernels that must agree bit for bit:
//   letterbox_kernel / lb_pixel inside the fused stem (tower_kernels.hip) and augment_letterbox_kernel (augment_kernels.hip).
// Everything here has internal linkage: each translation unit compiles its own copy of the same expressions.
#pragma once
#include "kernels.h"

namespace fv {
namespace {

struct LbParams {
  const void* img; bf16_t* pix; int dtype, B, C, Hin, Win, S, rh, rw, pt, pl; float pad, sh, sw;
};

__device__ __forceinline__ float lb_fetch(const LbParams& p, size_t plane, int y, int x) {
  const size_t i = plane + (size_t)y * p.Win + x;
  return p.dtype == FV_U8 ? (float)static_cast<const uint8_t*>(p.img)[i] : static_cast<const float*>(p.img)[i];
}

// every product and sum is rounded on its own (fp contract off: HIP's __f*_rn are plain operators and would still fuse), so that the
// kernels that evaluate these expressions -- letterbox_kernel, lb_pixel inside the stem and the augmented letterbox -- agree bit for bit
// whatever hipcc would have contracted to an fma in either context
__device__ __forceinline__ float lb_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
  return (1.0f - w) * a + w * b;
}
__device__ __forceinline__ float lb_src(int d, float scale) {
#pragma clang fp contract(off)
  return fmaxf(((float)d + 0.5f) * scale - 0.5f, 0.0f);
}
__device__ __forceinline__ float lb_frac(float s, int i) {
#pragma clang fp contract(off)
  return s - (float)i;
}

// One thread = one output column x LB_R consecutive output rows: when upscaling (the path's case: 336 -> 1024, ~3 output rows per
// source row) consecutive rows share their two source rows, so the 4 taps x 3 channels are fetched again only when y0 moves -- a
// third of the loads and of the x arithmetic of the one-pixel-per-thread form, the same values bit for bit.
constexpr int LB_R = 4;

// geometry of reference resize_with_pad (model/fastvlm_adapter.py:36-55) for one call; shared by the letterbox kernels and the stem
// that samples the source image itself
inline int lb_params(const void* img, int dtype, int B, int C, int Hin, int Win, int S, float pad_value, int letterbox, bf16_t* pix, LbParams& p) {
  if (B <= 0 || Hin <= 0 || Win <= 0 || S <= 0) return fv_fail(FV_ERR_ARG, "letterbox: empty shape");
  if (C != 1 && C != 3 && C != 4) return fv_fail(FV_ERR_ARG, "letterbox: C must be 1, 3 or 4 (got %d)", C);
  if (dtype != FV_F32 && dtype != FV_U8) return fv_fail(FV_ERR_ARG, "letterbox: dtype must be f32 or u8");
  p.img = img; p.pix = pix; p.dtype = dtype; p.B = B; p.C = C; p.Hin = Hin; p.Win = Win; p.S = S; p.pad = pad_value;
  if (letterbox) {
    // reference: ratio = max(W/S, H/S); resized = int(dim / ratio) in Python double arithmetic
    const double ratio = ((double)Win / S > (double)Hin / S) ? (double)Win / S : (double)Hin / S;
    p.rh = (int)((double)Hin / ratio);
    p.rw = (int)((double)Win / ratio);
    if (p.rh > S || p.rw > S || p.rh < 1 || p.rw < 1) return fv_fail(FV_ERR_ARG, "letterbox: degenerate resize %dx%d", p.rh, p.rw);
  } else {
    p.rh = S; p.rw = S;
  }
  p.pt = S - p.rh; p.pl = S - p.rw;
  p.sh = (float)Hin / (float)p.rh;
  p.sw = (float)Win / (float)p.rw;
  return FV_OK;
}

}  // namespace
}  // namespace fv
