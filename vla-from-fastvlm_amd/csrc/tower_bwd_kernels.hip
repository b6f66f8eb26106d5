// tower_bwd_kernels.hip -- backward kernels of the FastViT-HD tower (second slice: the tower trainable).
//
// The reference never differentiates the tower (model/fastvlm_adapter.py:501 is an unconditional no_grad; the knob it nominally has is
// fastvla/configuration_fastvla.py:23 `freeze_backbone`, applied at model/fastvlm_adapter.py:170-173): the arithmetic here is torch autograd's
// over the inference-form graph oracle/fastvit_hd.py restates (every gradient checked against it, tests/test_gpu_train_tower.py).
//
// Conventions.  Activations NHWC bf16 as the forward leaves them; every gradient tensor NHWC fp16 carrying the loss scale of
// fv_train_set_options (saturating casts); weight gradients fp32, summed in a FIXED order (per-block partial sums + one reduce pass, no
// atomics: bit-repeatable).  The dense contractions (1x1 convs) run on the GEMM kernels of gemm_bf16.hip (FV_EPI_GELU_GRAD / MUL_AUX / F16
// epilogues, TN instance for the weight gradients); this file holds what is left:
//   dw_dgrad_kernel / dw_wgrad_kernel   depthwise k x k (stride 1 / 2, channel multiplier 1 / 2): input gradient (+ residual), tap + bias gradients
//   ln_bwd_kernel                       LayerNormChannel (rows of C)
//   tattn_dq_kernel / tattn_dkv_kernel  non-causal head_dim-32 attention on v_mfma_f32_16x16x32_f16 (row statistics recomputed: any token count)
//   se_*                                conv_exp's squeeze-excite + GELU
//   stem0_wgrad_kernel                  the dense 3x3 stride-2 stem conv (pre-activation recomputed from the pixels)
//   colsum16 / partial_reduce / ls_grads / mul / gelu_grad_mul / tower_commit  HBM-bound glue
#include <algorithm>

#include "kernels.h"

namespace fv {
namespace {

__device__ __forceinline__ float h2f_lo(uint32_t u) { return (float)__builtin_bit_cast(f16x2, u)[0]; }
__device__ __forceinline__ float h2f_hi(uint32_t u) { return (float)__builtin_bit_cast(f16x2, u)[1]; }

// ------------------------------------------------------------------------------------------------ depthwise: input gradient
// dx[b][yi][xi][ci] = (res) + sum_{q < MULT} sum_{ky, kx} w[ky K + kx][ci MULT + q] dy[b][yo][xo][ci MULT + q],  yo S = yi + PAD - ky, xo S = xi + PAD - kx
// block = one slab of CS input channels (weights of the slab in LDS) x a run of pixels; thread = 8 input channels of one pixel
template <int K, int S, int MULT>
__global__ __launch_bounds__(256) void dw_dgrad_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ w, const bf16_t* __restrict__ res,
                                                        bf16_t* __restrict__ dx, int Hi, int Wi, int Ci, int Ho, int Wo, int CS, int nslabs, long npix,
                                                        int iters, unsigned* sat, int round_w) {
  constexpr int PAD = K / 2;
  extern __shared__ __attribute__((aligned(16))) float sw_dg[];   // [K*K][CS * MULT]
  const int slab = blockIdx.x % nslabs;
  const long pblock = blockIdx.x / nslabs;
  const int Co = Ci * MULT, cw = CS * MULT;
  // round_w: the forward ran this layer on the MFMA depthwise kernels, whose Toeplitz tables hold the taps rounded to bf16 -- the backward differentiates THAT function
  for (int i = threadIdx.x; i < K * K * cw; i += 256) {
    const float wv = w[(size_t)(i / cw) * Co + slab * cw + (i % cw)];
    sw_dg[i] = round_w ? bf2f(f2bf(wv)) : wv;
  }
  __syncthreads();
  const int G = CS >> 3, ppb = 256 / G;
  const int g = threadIdx.x % G, pl = threadIdx.x / G;
  if (pl >= ppb) return;
  const int ci0 = slab * CS + g * 8;
  for (int it = 0; it < iters; ++it) {
    const long p = (pblock * iters + it) * ppb + pl;
    if (p >= npix) return;
    const int xi = (int)(p % Wi);
    const long t = p / Wi;
    const int yi = (int)(t % Hi);
    const long b = t / Hi;
    float acc[8];
    if (res) {
      unpack8_h(*reinterpret_cast<const uint4*>(res + p * Ci + ci0), acc);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    }
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky) {
      const int yy = yi + PAD - ky;
      if (S == 2 && (yy & 1)) continue;
      const int yo = S == 2 ? (yy >> 1) : yy;
      if (yo < 0 || yo >= Ho) continue;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int xx = xi + PAD - kx;
        if (S == 2 && (xx & 1)) continue;
        const int xo = S == 2 ? (xx >> 1) : xx;
        if (xo < 0 || xo >= Wo) continue;
        const bf16_t* dp = dy + ((b * Ho + yo) * Wo + xo) * (long)Co + (long)ci0 * MULT;
        const float* wp = sw_dg + (ky * K + kx) * cw + g * 8 * MULT;
        if (MULT == 1) {
          float v[8];
          unpack8_h(*reinterpret_cast<const uint4*>(dp), v);
          const float4 w0 = *reinterpret_cast<const float4*>(wp), w1 = *reinterpret_cast<const float4*>(wp + 4);
          acc[0] += w0.x * v[0]; acc[1] += w0.y * v[1]; acc[2] += w0.z * v[2]; acc[3] += w0.w * v[3];
          acc[4] += w1.x * v[4]; acc[5] += w1.y * v[5]; acc[6] += w1.z * v[6]; acc[7] += w1.w * v[7];
        } else {
          float v[16];
          unpack8_h(*reinterpret_cast<const uint4*>(dp), v);
          unpack8_h(*reinterpret_cast<const uint4*>(dp + 8), v + 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += wp[2 * e] * v[2 * e] + wp[2 * e + 1] * v[2 * e + 1];
        }
      }
    }
    count_f16_sat8(acc, sat);
    *reinterpret_cast<uint4*>(dx + p * Ci + ci0) = pack8_h(acc);
  }
}

// ------------------------------------------------------------------------------------------------ depthwise: tap + bias gradients
// part[pb][t][co] = sum over the block's output pixels of dy[pix][co] x[pix S - PAD + tap t][co / MULT]  (t = K*K: the bias gradient, x = 1)
// thread = one output-channel PAIR x a slice of the block's pixels; K*K + 1 accumulator pairs in registers; slices folded through LDS in a fixed order
template <int K, int S, int MULT>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part, int Hi, int Wi,
                                                        int Ci, int Ho, int Wo, int CS, int nslabs, long npix, long ppb) {
  constexpr int PAD = K / 2, NT = K * K + 1, RT = 10;   // RT taps per LDS fold round
  extern __shared__ __attribute__((aligned(16))) float sr_wg[];   // [RT][NPS][CS]
  const int slab = blockIdx.x % nslabs;
  const long pb = blockIdx.x / nslabs;
  const int Co = Ci * MULT, hp = CS >> 1, NPS = 256 / hp;
  const int cp = threadIdx.x % hp, ps = threadIdx.x / hp;
  const int co = slab * CS + 2 * cp;
  float a0[NT], a1[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { a0[t] = 0.f; a1[t] = 0.f; }
  if (ps < NPS) {
    const long p1 = pb * ppb + ppb < npix ? pb * ppb + ppb : npix;
    for (long p = pb * ppb + ps; p < p1; p += NPS) {
      const int xo = (int)(p % Wo);
      const long t2 = p / Wo;
      const int yo = (int)(t2 % Ho);
      const long b = t2 / Ho;
      const uint32_t du = *reinterpret_cast<const uint32_t*>(dy + p * Co + co);
      const float d0 = h2f_lo(du), d1 = h2f_hi(du);
      a0[K * K] += d0; a1[K * K] += d1;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int iy = yo * S - PAD + ky;
        if (iy < 0 || iy >= Hi) continue;
        const bf16_t* rowp = x + ((b * Hi + iy) * (long)Wi) * Ci + (MULT == 1 ? co : (co >> 1));
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int ix = xo * S - PAD + kx;
          if (ix < 0 || ix >= Wi) continue;
          if (MULT == 1) {
            const uint32_t xu = *reinterpret_cast<const uint32_t*>(rowp + (long)ix * Ci);
            a0[ky * K + kx] += d0 * bf_lo(xu);
            a1[ky * K + kx] += d1 * bf_hi(xu);
          } else {
            const float xv = bf2f(rowp[(long)ix * Ci]);
            a0[ky * K + kx] += d0 * xv;
            a1[ky * K + kx] += d1 * xv;
          }
        }
      }
    }
  }
#pragma unroll
  for (int r0 = 0; r0 < NT; r0 += RT) {
    if (ps < NPS) {
#pragma unroll
      for (int t = 0; t < RT; ++t)
        if (r0 + t < NT) {
          sr_wg[(t * NPS + ps) * CS + 2 * cp] = a0[r0 + t];
          sr_wg[(t * NPS + ps) * CS + 2 * cp + 1] = a1[r0 + t];
        }
    }
    __syncthreads();
    const int nt = NT - r0 < RT ? NT - r0 : RT;
    for (int i = threadIdx.x; i < nt * CS; i += 256) {
      const int t = i / CS, c = i % CS;
      float s = 0.f;
      for (int q = 0; q < NPS; ++q) s += sr_wg[(t * NPS + q) * CS + c];
      part[((size_t)pb * NT + r0 + t) * Co + slab * CS + c] = s;
    }
    __syncthreads();
  }
}

// The stride-1, multiplier-1 form (every RepMixer 3x3, ConvFFN / RepCPE 7x7: 99 % of the tap-gradient work), register-blocked: a thread owns one channel
// PAIR and walks whole output rows in chunks of 8 pixels -- for each kernel row ky it loads the 8 + K - 1 input values and the 8 gradient values once and does
// 8 K packed FMAs on them (no per-tap address arithmetic, no integer division in the loop).  part[rb][t][c] as dw_wgrad_kernel.
template <int K, int S = 1, int MULT = 1>   // H, W: the INPUT map; C: OUTPUT channels (input channel of output channel co: co / MULT); nrows = B * Ho output rows
__global__ __launch_bounds__(256) void dw_wgrad_rows_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part, int H, int W,
                                                             int C, int CS, int nslabs, int nrows, int rpb, int Ho, int Wo) {
  constexpr int PAD = K / 2, NT = K * K + 1, RT = 10, R = 8, NX = (R - 1) * S + K;
  extern __shared__ __attribute__((aligned(16))) float sr_wr[];   // [RT][NPS][CS]
  const int slab = blockIdx.x % nslabs;
  const int rb = blockIdx.x / nslabs;
  const int hp = CS >> 1, NPS = 256 / hp;
  const int cp = threadIdx.x % hp, ps = threadIdx.x / hp;
  const int co = slab * CS + 2 * cp;
  f32x2 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x2{0.f, 0.f};
  if (ps < NPS) {
    const int r1 = (rb + 1) * rpb < nrows ? (rb + 1) * rpb : nrows;
    const int Ci = C / MULT, ci = co / MULT;
    for (int row = rb * rpb + ps; row < r1; row += NPS) {
      const int yo = row % Ho, b = row / Ho;
      const bf16_t* dyrow = dy + ((size_t)row * Wo) * C + co;
      for (int x0 = 0; x0 < Wo; x0 += R) {
        f32x2 d[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t u = x0 + r < Wo ? *reinterpret_cast<const uint32_t*>(dyrow + (size_t)(x0 + r) * C) : 0u;
          d[r] = f32x2{h2f_lo(u), h2f_hi(u)};
          acc[K * K] += d[r];
        }
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          const int iy = yo * S + ky - PAD;
          if (iy < 0 || iy >= H) continue;
          const bf16_t* xrow = x + (((size_t)b * H + iy) * W) * Ci + ci;
          f32x2 xv[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) {
            const int ix = x0 * S - PAD + i;
            const bool ok = ix >= 0 && ix < W;
            if (MULT == 1) {
              const uint32_t u = ok ? *reinterpret_cast<const uint32_t*>(xrow + (size_t)ix * Ci) : 0u;
              xv[i] = f32x2{bf_lo(u), bf_hi(u)};
            } else {   // both outputs of the pair read the same input channel
              const float v = ok ? bf2f(xrow[(size_t)ix * Ci]) : 0.f;
              xv[i] = f32x2{v, v};
            }
          }
#pragma unroll
          for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[ky * K + kx] = __builtin_elementwise_fma(d[r], xv[r * S + kx], acc[ky * K + kx]);
        }
      }
    }
  }
#pragma unroll
  for (int r0 = 0; r0 < NT; r0 += RT) {
    if (ps < NPS) {
#pragma unroll
      for (int t = 0; t < RT; ++t)
        if (r0 + t < NT) *reinterpret_cast<f32x2*>(&sr_wr[(t * NPS + ps) * CS + 2 * cp]) = acc[r0 + t];
    }
    __syncthreads();
    const int nt = NT - r0 < RT ? NT - r0 : RT;
    for (int i = threadIdx.x; i < nt * CS; i += 256) {
      const int t = i / CS, c = i % CS;
      float sm = 0.f;
      for (int q = 0; q < NPS; ++q) sm += sr_wr[(t * NPS + q) * CS + c];
      part[((size_t)rb * NT + r0 + t) * C + slab * CS + c] = sm;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ depthwise tap gradients on the matrix cores (round 6)
// dw[ky][kx][c] = sum_{b,r,q} dy[b][r][q][c] x[b][r + ky - P][q + kx - P][c] is, per channel, a correlation of two images: 49 (9) outputs, the contraction over ALL
// pixels.  v_mfma_f32_4x4x4_16B_f16 multiplies sixteen independent 4x4 blocks -- block = channel, as in the forward's Toeplitz kernels -- with
//     contraction k = 4 consecutive COLUMNS of an x quad Qx;  A_c[i][k] = x[r - P + 4 Rg + i][X0 + 4 Qx + k]        (i: four x rows, Rg in {0, 1})
//                                                            B_c[k][j] = dy[r][D0 + 4 Qx - (s + j) + k]             (j: four column shifts, s in {0, 4})
//     D_c[i][j] += A_c B_c = the contribution of dy row r / x quad Qx to tap (ky = 4 Rg + i, kx = s + j)            (X0 = strip - P, D0 = strip: the shift is K-free)
// 4 MFMAs per (dy row, x quad, 16 channels) cover the 8 x 8 tap slots of which 49 are the 7x7's (77 % useful); the 3x3 takes one (Rg = 0, s = 0).  A is an aligned
// cell of the x ring ([row][quad][channel][4 columns], the forward kernels' layout, x widened bf16 -> fp16 EXACTLY on its way into LDS); B is a 4-column window of the
// dy row that starts (s + j) columns to the left of the x quad -- a per-lane constant shift: two neighbouring dy cells, three v_cndmask and two v_perm -- and the s = 4
// window of quad Qx IS the s = 0 window of quad Qx - 1, so one window is built per (row, quad).  One block = (image, 32-column strip, 32-channel slice) marching down
// the map in units of 8 rows (x ring of 16 rows, one dy unit), accumulators live across the whole march; per-block partial sums, fixed-order reduce (no atomics).
// The bias gradient is summed from the dy tasks while they are in registers.
template <int K>
struct DwWgGeo {
  static constexpr int PAD = K / 2, NQX = (32 + 2 * PAD + 3) / 4, NQD = NQX + 2;   // x quads per ring row; dy cells per row: quads -2 .. NQX - 1 (only 0 .. 7 carry data)
  static constexpr int RSX = NQX * 256 + 64, RSD = NQD * 256 + 64;
  static constexpr int NS = K > 4 ? 2 : 1, NRG = K > 4 ? 2 : 1;
  static constexpr int LDS = 16 * RSX + 8 * RSD;
};
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_w;
typedef __attribute__((ext_vector_type(4))) short s16x4_w;
template <int K>
__global__ __launch_bounds__(256, 2) void dw_wgrad_mfma_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part, int H, int W, int C,
                                                                int tiles_x, int nslices) {
  using G = DwWgGeo<K>;
  constexpr int PAD = G::PAD, NQX = G::NQX, RSX = G::RSX, RSD = G::RSD, NS = G::NS, NRG = G::NRG, NT = K * K + 1;
  extern __shared__ __attribute__((aligned(16))) char wg_smem[];
  char* sX = wg_smem;                 // x ring: image row rho at ring row (rho - PAD) & 15
  char* sD = wg_smem + 16 * RSX;      // dy unit: row r & 7, cell index = quad + 2
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int slice = bid % nslices; bid /= nslices;
  const int tx = bid % tiles_x;
  const long b = bid / tiles_x;
  const int c0 = slice * 32;
  const int gg = wid & 1, rg = wid >> 1;          // wave = (16-channel group, 4 of the unit's 8 dy rows)
  const int bch = lane >> 2, jr = lane & 3;       // lane = (channel within the group, row i of A / shift j of B)
  const int ng = (H + 7) / 8;

  // ---- staging: tasks of 4 pixels x 8 channels, transposed in registers (v_perm) into the cell layout
  constexpr int NTX = 8 * NQX * 4, TPX = (NTX + 255) / 256;
  uint4 px[TPX][4], pd[4];
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#define WG_LOAD_X(U)                                                                                             \
  {                                                                                                              \
    _Pragma("unroll") for (int tt = 0; tt < TPX; ++tt) {                                                         \
      const int task = tid + 256 * tt;                                                                           \
      const int cg = task & 3, quad = (task >> 2) % NQX, row = (task >> 2) / NQX;                                \
      const int iy = 8 * (U) + PAD + row, ix0 = tx * 32 - PAD + quad * 4;                                        \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                            \
        const int ix = ix0 + j;                                                                                  \
        px[tt][j] = (task < NTX && iy >= 0 && iy < H && ix >= 0 && ix < W)                                       \
                        ? *reinterpret_cast<const uint4*>(x + (((size_t)b * H + iy) * W + ix) * C + c0 + cg * 8)  \
                        : make_uint4(0, 0, 0, 0);                                                                \
      }                                                                                                          \
    }                                                                                                            \
  }
#define WG_LOAD_D(U)                                                                                             \
  {                                                                                                              \
    const int cg = tid & 3, quad = (tid >> 2) & 7, row = tid >> 5;                                               \
    const int iy = 8 * (U) + row, ix0 = tx * 32 + quad * 4;                                                      \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                              \
      const int ix = ix0 + j;                                                                                    \
      pd[j] = ((U) < ng && iy < H && ix < W) ? *reinterpret_cast<const uint4*>(dy + (((size_t)b * H + iy) * W + ix) * C + c0 + cg * 8) : make_uint4(0, 0, 0, 0); \
    }                                                                                                            \
  }
  // bf16 pair (one dword) -> the same two values as fp16 (exact: 8 significant bits; activations far inside fp16's range)
  auto bf2h = [](uint32_t u) -> uint32_t { return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u))); };
#define WG_WRITE_X(U)                                                                                            \
  {                                                                                                              \
    _Pragma("unroll") for (int tt = 0; tt < TPX; ++tt) {                                                         \
      const int task = tid + 256 * tt;                                                                           \
      if (task < NTX) {                                                                                          \
        const int cg = task & 3, quad = (task >> 2) % NQX, row = (task >> 2) / NQX;                              \
        const uint32_t d[4][4] = {{px[tt][0].x, px[tt][0].y, px[tt][0].z, px[tt][0].w}, {px[tt][1].x, px[tt][1].y, px[tt][1].z, px[tt][1].w}, \
                                  {px[tt][2].x, px[tt][2].y, px[tt][2].z, px[tt][2].w}, {px[tt][3].x, px[tt][3].y, px[tt][3].z, px[tt][3].w}}; \
        const uint32_t dst = (uint32_t)((8 * ((U) & 1) + row) * RSX + quad * 256 + cg * 64) | (uint32_t)((((quad & 3) << 1) | (cg >> 1)) << 3); \
        _Pragma("unroll") for (int dd = 0; dd < 4; ++dd) {                                                       \
          uint2 ev, od;                                                                                          \
          ev.x = bf2h(__builtin_amdgcn_perm(d[1][dd], d[0][dd], 0x05040100u));                                   \
          ev.y = bf2h(__builtin_amdgcn_perm(d[3][dd], d[2][dd], 0x05040100u));                                   \
          od.x = bf2h(__builtin_amdgcn_perm(d[1][dd], d[0][dd], 0x07060302u));                                   \
          od.y = bf2h(__builtin_amdgcn_perm(d[3][dd], d[2][dd], 0x07060302u));                                   \
          *reinterpret_cast<uint2*>(sX + (dst ^ (uint32_t)((2 * dd) * 8))) = ev;                                 \
          *reinterpret_cast<uint2*>(sX + (dst ^ (uint32_t)((2 * dd + 1) * 8))) = od;                             \
        }                                                                                                        \
      }                                                                                                          \
    }                                                                                                            \
  }
#define WG_WRITE_D()                                                                                             \
  {                                                                                                              \
    const int cg = tid & 3, quad = (tid >> 2) & 7, row = tid >> 5, qc = quad + 2;                                \
    const uint32_t d[4][4] = {{pd[0].x, pd[0].y, pd[0].z, pd[0].w}, {pd[1].x, pd[1].y, pd[1].z, pd[1].w},         \
                              {pd[2].x, pd[2].y, pd[2].z, pd[2].w}, {pd[3].x, pd[3].y, pd[3].z, pd[3].w}};        \
    const uint32_t dst = (uint32_t)(row * RSD + qc * 256 + cg * 64) | (uint32_t)((((qc & 3) << 1) | (cg >> 1)) << 3); \
    _Pragma("unroll") for (int dd = 0; dd < 4; ++dd) {                                                           \
      uint2 ev, od;                                                                                              \
      ev.x = __builtin_amdgcn_perm(d[1][dd], d[0][dd], 0x05040100u);                                             \
      ev.y = __builtin_amdgcn_perm(d[3][dd], d[2][dd], 0x05040100u);                                             \
      od.x = __builtin_amdgcn_perm(d[1][dd], d[0][dd], 0x07060302u);                                             \
      od.y = __builtin_amdgcn_perm(d[3][dd], d[2][dd], 0x07060302u);                                             \
      *reinterpret_cast<uint2*>(sD + (dst ^ (uint32_t)((2 * dd) * 8))) = ev;                                     \
      *reinterpret_cast<uint2*>(sD + (dst ^ (uint32_t)((2 * dd + 1) * 8))) = od;                                 \
      /* the bias gradient: this thread's 8 channels, 4 pixels each */                                           \
      bsum[2 * dd] += (h2f_lo(d[0][dd]) + h2f_lo(d[1][dd])) + (h2f_lo(d[2][dd]) + h2f_lo(d[3][dd]));             \
      bsum[2 * dd + 1] += (h2f_hi(d[0][dd]) + h2f_hi(d[1][dd])) + (h2f_hi(d[2][dd]) + h2f_hi(d[3][dd]));         \
    }                                                                                                            \
  }
  // the dy cells outside the strip (quads -2, -1 and 8 .. NQX - 1) are zero for the whole march
  for (int i = tid; i < 8 * (G::NQD - 8) * 32; i += 256) {
    const int ch = i & 31, z = (i >> 5) % (G::NQD - 8), row = (i >> 5) / (G::NQD - 8);
    const int qc = z < 2 ? z : z + 8;
    *reinterpret_cast<uint2*>(sD + row * RSD + qc * 256 + ch * 8) = make_uint2(0u, 0u);
  }
  uint32_t sw[4];   // the lane's swizzled channel offsets (one per cell index & 3)
#pragma unroll
  for (int v = 0; v < 4; ++v) sw[v] = (uint32_t)(((gg * 16 + bch) ^ ((v << 1) | gg)) << 3);
  // per-lane window selectors: shift j = jr -> the window starts 4 - j columns into [cell Q - 1 | cell Q] (j = 0: the cell Q itself)
  const bool j0 = jr == 0, j3 = jr == 3;
  const uint32_t selw = (jr & 1) ? 0x05040302u : 0x03020100u;

  f32x4 acc[NS][NRG];
#pragma unroll
  for (int sI = 0; sI < NS; ++sI)
#pragma unroll
    for (int r = 0; r < NRG; ++r) acc[sI][r] = f32x4{0.f, 0.f, 0.f, 0.f};

  WG_LOAD_X(-1)
  WG_WRITE_X(-1)
  WG_LOAD_X(0)
  WG_WRITE_X(0)
  WG_LOAD_D(0)
  WG_WRITE_D()
  if (ng > 1) { WG_LOAD_X(1) WG_LOAD_D(1) }
  for (int g = 0; g < ng; ++g) {
    __syncthreads();   // x units g - 1, g and dy unit g are in LDS
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int lr = rg * 4 + rr;                                   // dy row within the unit; image row r = 8 g + lr
      const char* drow = sD + lr * RSD;
      uint32_t xrow[NRG];                                           // ring row of the lane's x row: image row r - PAD + 4 Rg + i -> (r - 2 PAD + 4 Rg + i) & 15
#pragma unroll
      for (int r = 0; r < NRG; ++r) xrow[r] = (uint32_t)((8 * g + lr - 2 * PAD + 4 * r + jr) & 15) * RSX;
      uint2 cprev = *reinterpret_cast<const uint2*>(drow + sw[1] + 1 * 256);   // dy quad -1 (cell 1): zero
      s16x4_w bprev = {0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < NQX; ++q) {
        const uint2 cq = *reinterpret_cast<const uint2*>(drow + sw[(q + 2) & 3] + (q + 2) * 256);   // dy quad q
        // window of shift j over [cprev | cq] = dwords d0 d1 d2 d3: j = 0: (d2, d3); 1: d1 d2 d3 >> 16; 2: (d1, d2); 3: d0 d1 d2 >> 16
        const uint32_t e0 = j3 ? cprev.x : (j0 ? cq.x : cprev.y);
        const uint32_t e1 = j3 ? cprev.y : (j0 ? cq.y : cq.x);
        const uint32_t e2 = j3 ? cq.x : cq.y;
        uint2 wv;
        wv.x = __builtin_amdgcn_perm(e1, e0, selw);
        wv.y = __builtin_amdgcn_perm(e2, e1, selw);
        const s16x4_w bq = __builtin_bit_cast(s16x4_w, wv);
#pragma unroll
        for (int r = 0; r < NRG; ++r) {
          const s16x4_w a = __builtin_bit_cast(s16x4_w, *reinterpret_cast<const uint2*>(sX + xrow[r] + sw[q & 3] + q * 256));
          acc[0][r] = __builtin_amdgcn_mfma_f32_4x4x4f16(__builtin_bit_cast(f16x4_w, a), __builtin_bit_cast(f16x4_w, bq), acc[0][r], 0, 0, 0);
          if (NS > 1) acc[NS - 1][r] = __builtin_amdgcn_mfma_f32_4x4x4f16(__builtin_bit_cast(f16x4_w, a), __builtin_bit_cast(f16x4_w, bprev), acc[NS - 1][r], 0, 0, 0);
        }
        cprev = cq;
        bprev = bq;
      }
    }
    __syncthreads();   // every wave is done with x unit g - 1 and dy unit g
    if (g + 1 < ng) { WG_WRITE_X(g + 1) WG_WRITE_D() }
    if (g + 2 < ng) { WG_LOAD_X(g + 2) WG_LOAD_D(g + 2) }
  }
  __syncthreads();
  // ---- fold: the two row-half waves of a channel group add up; then part[(blk * NT + t) * C + c]; bias sums over the 64 threads of a channel group of 8
  float* sF = reinterpret_cast<float*>(wg_smem);   // [wave 4][lane 64][NS * NRG * 4] taps, then [256][8] bias
  constexpr int NV = NS * NRG * 4;
#pragma unroll
  for (int sI = 0; sI < NS; ++sI)
#pragma unroll
    for (int r = 0; r < NRG; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) sF[(wid * 64 + lane) * NV + (sI * NRG + r) * 4 + i] = acc[sI][r][i];
  float* sB = sF + 4 * 64 * NV;
#pragma unroll
  for (int e = 0; e < 8; ++e) sB[tid * 8 + e] = bsum[e];
  __syncthreads();
  const size_t blk = (size_t)b * tiles_x + tx;
  for (int o = tid; o < 2 * 64 * NV; o += 256) {
    const int v = o % NV, ln = (o / NV) & 63, g2 = o / (NV * 64);
    const int i = v & 3, r = (v >> 2) % NRG, sI = (v >> 2) / NRG;
    const int ky = 4 * r + i, kx = 4 * sI + (ln & 3);
    if (ky < K && kx < K) {
      const float sum = sF[((g2 + 0) * 64 + ln) * NV + v] + sF[((g2 + 2) * 64 + ln) * NV + v];
      part[(blk * NT + ky * K + kx) * C + c0 + g2 * 16 + (ln >> 2)] = sum;
    }
  }
  if (tid < 32) {   // channel c0 + tid = group cg = tid / 8, element tid % 8: the threads with (t & 3) == cg hold its sums, added in thread order
    const int cg = tid >> 3, e = tid & 7;
    float sum = 0.f;
    for (int t = cg; t < 256; t += 4) sum += sB[t * 8 + e];
    part[(blk * NT + K * K) * C + c0 + tid] = sum;
  }
#undef WG_LOAD_X
#undef WG_LOAD_D
#undef WG_WRITE_X
#undef WG_WRITE_D
}

// out[i] = sum_p part[p * stride + i] (fixed order), i < n; the first n1 results go to out1, the rest to out2 (taps | bias, dw | db ...)
// The same stride-1 form with the INPUT tile staged through LDS (round 5; the default): the register-blocked kernel above reads every input row K times from
// global memory with two waves per SIMD to hide it behind -- it ran at 1/12 of its packed-FMA time.  Here a block = CS channels x NPS consecutive output rows of
// one image; per 8-column chunk the (NPS + K - 1) x (8 + K - 1) input pixels of the slab go global -> registers -> LDS once (the next chunk's loads in flight
// under the current chunk's FMAs), every thread reads its K x (8 + K - 1) window as conflict-free dwords, out-of-map pixels are stored as zeros (no bounds
// checks in the FMA loop).  part[block][t][c] as above.
template <int K, int S = 1, int MULT = 1>   // H, W: the INPUT map; C: OUTPUT channels (CS of them per block, reading CS / MULT input channels); Ho, Wo: the output map
__global__ __launch_bounds__(256, 2) void dw_wgrad_lds_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, float* __restrict__ part, int H, int W,
                                                               int C, int CS, int nslabs, int ngroups, int gpb, int gpi, unsigned xbytes, int Ho, int Wo) {
  constexpr int PAD = K / 2, NT = K * K + 1, RT = 10, R = 8, NC = (R - 1) * S + K;
  constexpr int MAXP = 10;                              // 16-byte pieces per thread: NR * NC * CS / 8 / 256 <= (4 + 6) * 14 * 16 / 256 = 8.75
  extern __shared__ __attribute__((aligned(16))) char sm_wl[];   // two input tiles [NR][NC][CS] bf16 (MAXP * 4 KB each), reused at the end as the fold scratch [RT][NPS][CS] f32
  float* sR = reinterpret_cast<float*>(sm_wl);
  const int slab = blockIdx.x % nslabs;
  const int gb = blockIdx.x / nslabs;
  const int hp = CS >> 1, NPS = 256 / hp, NR = (NPS - 1) * S + K;
  const int Ci = C / MULT, CSi = CS / MULT;
  const int cp = threadIdx.x % hp, ps = threadIdx.x / hp;
  const int co = slab * CS + 2 * cp;
  const int c8n = CSi >> 3, nchunk16 = NR * NC * c8n;   // 16-byte pieces of a tile
  const int wv = threadIdx.x >> 6;
  f32x2 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x2{0.f, 0.f};
  const int g1 = (gb + 1) * gpb < ngroups ? (gb + 1) * gpb : ngroups;
  const int ncx = (Wo + R - 1) / R;
  // the tile goes global -> LDS by LDS-DMA (no staging registers next to the 100 accumulators): piece idx = (pixel slot, 8-channel group) lands at byte 16 idx;
  // pixels outside the map read past the descriptor's range and arrive as zeros
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(x), 0, xbytes, 0x00020000);
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  auto issue = [&](int g, int cx, int buf) {
    const int b = g / gpi, yb = (g % gpi) * NPS, x0 = cx * R;
    char* base = sm_wl + buf * (MAXP * 4096);
#pragma unroll
    for (int q = 0; q < MAXP; ++q) {
      if (q * 256 + wv * 64 < nchunk16) {   // wave-uniform
        const int idx = threadIdx.x + 256 * q;
        const int c8 = idx % c8n, slot = idx / c8n;
        const int col = slot % NC, row = slot / NC;
        const int iy = yb * S - PAD + row, ix = x0 * S - PAD + col;
        const bool ok = idx < nchunk16 && iy >= 0 && iy < H && ix >= 0 && ix < W;
        const uint32_t off = ok ? (uint32_t)(((((size_t)b * H + iy) * W + ix) * Ci + slab * CSi + c8 * 8) * 2) : 0xfffffff0u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr_t)(base + (q * 256 + wv * 64) * 16), 16, off, 0, 0, 0);
      }
    }
  };
  auto load_d = [&](int g, int cx, uint32_t (&dn)[R]) {
    const int b = g / gpi, yo = (g % gpi) * NPS + ps, x0 = cx * R;
    const bool rowok = ps < NPS && yo < Ho;
    const bf16_t* dyrow = dy + (((size_t)b * Ho + (rowok ? yo : 0)) * Wo) * C + co;
#pragma unroll
    for (int r = 0; r < R; ++r) dn[r] = (rowok && x0 + r < Wo) ? *reinterpret_cast<const uint32_t*>(dyrow + (size_t)(x0 + r) * C) : 0u;
  };
  int g = gb * gpb, cx = 0, buf = 0;
  uint32_t dcur[R], dnext[R];
  if (g < g1) { issue(g, 0, 0); load_d(g, 0, dcur); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  while (g < g1) {
    int gn = g, cxn = cx + 1;
    if (cxn == ncx) { cxn = 0; gn = g + 1; }
    const bool more = gn < g1;
    if (more) { issue(gn, cxn, buf ^ 1); load_d(gn, cxn, dnext); }
    {
      const bf16_t* sX = reinterpret_cast<const bf16_t*>(sm_wl + buf * (MAXP * 4096));
      if (ps < NPS) {
        f32x2 d[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          d[r] = f32x2{h2f_lo(dcur[r]), h2f_hi(dcur[r])};
          acc[K * K] += d[r];
        }
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          f32x2 xv[NC];
#pragma unroll
          for (int i = 0; i < NC; ++i) {
            if (MULT == 1) {
              const uint32_t u = *reinterpret_cast<const uint32_t*>(sX + ((size_t)((ps * S + ky) * NC + i)) * CSi + 2 * cp);
              xv[i] = f32x2{bf_lo(u), bf_hi(u)};
            } else {   // both outputs of the pair read the same input channel
              const float v = bf2f(sX[((size_t)((ps * S + ky) * NC + i)) * CSi + cp]);
              xv[i] = f32x2{v, v};
            }
          }
#pragma unroll
          for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[ky * K + kx] = __builtin_elementwise_fma(d[r], xv[r * S + kx], acc[ky * K + kx]);
          __builtin_amdgcn_sched_barrier(0);   // one kernel row's window at a time (hoisting the next rows' LDS reads over these FMAs spills)
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next tile (and the next gradient values) have landed ...
    __syncthreads();                                     // ... for everybody, and nobody still reads this one
#pragma unroll
    for (int r = 0; r < R; ++r) dcur[r] = dnext[r];
    g = gn; cx = cxn; buf ^= 1;
  }
#pragma unroll
  for (int r0 = 0; r0 < NT; r0 += RT) {
    if (ps < NPS) {
#pragma unroll
      for (int t = 0; t < RT; ++t)
        if (r0 + t < NT) *reinterpret_cast<f32x2*>(&sR[(t * NPS + ps) * CS + 2 * cp]) = acc[r0 + t];
    }
    __syncthreads();
    const int nt = NT - r0 < RT ? NT - r0 : RT;
    for (int i = threadIdx.x; i < nt * CS; i += 256) {
      const int t = i / CS, c = i % CS;
      float sm = 0.f;
      for (int q = 0; q < NPS; ++q) sm += sR[(t * NPS + q) * CS + c];
      part[((size_t)gb * NT + r0 + t) * C + slab * CS + c] = sm;
    }
    __syncthreads();
  }
}

// (a block = 64 outputs x 4 part lanes: each lane sums every fourth partial in order, the four are folded in order -- a fixed association)
__global__ __launch_bounds__(256) void partial_reduce_kernel(const float* __restrict__ part, long nparts, long stride, long n, long n1, float* __restrict__ out1,
                                                              float* __restrict__ out2, float scale) {
  __shared__ float sp[4][64];
  const int li = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + li;
  float s = 0.f;
  if (i < n)
    for (long p = pl; p < nparts; p += 4) s += part[p * stride + i];
  sp[pl][li] = s;
  __syncthreads();
  if (pl == 0 && i < n) {
    s = ((sp[0][li] + sp[1][li]) + (sp[2][li] + sp[3][li])) * scale;
    if (i < n1) out1[i] = s;
    else out2[i - n1] = s;
  }
}

// ------------------------------------------------------------------------------------------------ column sums of fp16 rows
// part[chunk][c] = sum of rows [chunk * rpc, ...) of in (fp16 [R][ld]); grid (ceil(C / 256), nchunks).  ncg = 8-column groups a block covers (<= 32): the
// other 256 / ncg thread rows walk the chunk's rows interleaved (at C = 96 a fixed 32 x 8 shape left 20 of 32 column lanes idle: 1.4 TB/s)
__global__ __launch_bounds__(256) void colsum16_kernel(const bf16_t* __restrict__ in, int ld, long R, int C, float* __restrict__ part, long rpc, int ncg) {
  __shared__ float sr[256 * 8];
  const int nty = 256 / ncg;
  const int tx = threadIdx.x % ncg, ty = threadIdx.x / ncg;
  const int c0 = blockIdx.x * 256 + tx * 8;
  const long r0 = (long)blockIdx.y * rpc, r1 = r0 + rpc < R ? r0 + rpc : R;
  float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c0 < C && ty < nty) {
    for (long r = r0 + ty; r < r1; r += nty) {
      float v[8];
      unpack8_h(*reinterpret_cast<const uint4*>(in + r * ld + c0), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += v[e];
    }
  }
  if (ty < nty) {
#pragma unroll
    for (int e = 0; e < 8; ++e) sr[ty * (ncg * 8) + tx * 8 + e] = a[e];
  }
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C && (int)threadIdx.x < ncg * 8) {
    float t = 0.f;
    for (int q = 0; q < nty; ++q) t += sr[q * (ncg * 8) + threadIdx.x];
    part[(size_t)blockIdx.y * C + c] = t;
  }
}

// ------------------------------------------------------------------------------------------------ elementwise
__global__ __launch_bounds__(256) void mul16_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, bf16_t* __restrict__ out, long n8, unsigned* sat) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float x[8], y[8];
  unpack8_h(*reinterpret_cast<const uint4*>(a + i * 8), x);
  unpack8_h(*reinterpret_cast<const uint4*>(b + i * 8), y);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] *= y[e];
  count_f16_sat8(x, sat);
  *reinterpret_cast<uint4*>(out + i * 8) = pack8_h(x);
}
// out f16 = dh f16 * gelu'(a bf16)
__global__ __launch_bounds__(256) void gelu_grad_mul_kernel(const bf16_t* __restrict__ dh, const bf16_t* __restrict__ pre, bf16_t* __restrict__ out, long n8, unsigned* sat) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float x[8], a[8];
  unpack8_h(*reinterpret_cast<const uint4*>(dh + i * 8), x);
  unpack8(*reinterpret_cast<const uint4*>(pre + i * 8), a);
  float dg8[8];
  gelu_and_grad8(a, dg8);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] *= dg8[e];
  count_f16_sat8(x, sat);
  *reinterpret_cast<uint4*>(out + i * 8) = pack8_h(x);
}
__global__ __launch_bounds__(256) void f16_to_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, long n8, float scale) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float x[8];
  unpack8_h(*reinterpret_cast<const uint4*>(in + i * 8), x);
  *reinterpret_cast<float4*>(out + i * 8) = make_float4(x[0] * scale, x[1] * scale, x[2] * scale, x[3] * scale);
  *reinterpret_cast<float4*>(out + i * 8 + 4) = make_float4(x[4] * scale, x[5] * scale, x[6] * scale, x[7] * scale);
}

// columns [C, C + 8) of fp16 rows [R][ld] <- {1, 0, ..., 0}: the ones column that makes a TN weight gradient deliver its bias gradient too
__global__ __launch_bounds__(256) void ones_col_kernel(bf16_t* __restrict__ out, int ld, int C, long R) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  *reinterpret_cast<uint4*>(out + r * ld + C) = make_uint4(0x00003c00u, 0u, 0u, 0u);   // fp16 1.0 = 0x3c00
}
__global__ __launch_bounds__(256) void scale_to_f16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, long n8, float scale, unsigned* sat) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const float4 a = *reinterpret_cast<const float4*>(in + i * 8), b = *reinterpret_cast<const float4*>(in + i * 8 + 4);
  float x[8] = {a.x * scale, a.y * scale, a.z * scale, a.w * scale, b.x * scale, b.y * scale, b.z * scale, b.w * scale};
  count_f16_sat8(x, sat);
  *reinterpret_cast<uint4*>(out + i * 8) = pack8_h(x);
}

// ---- the tower's own gradient scale.  dL/d(tower_out) of a B = 32 step has a median of 1e-3 x the loss scale and 4 % fp16 subnormals, and the gradient thins out
// further on its way to the 256 x 256 maps (the attention blocks' dS = P (dP - delta) is another 1e-3): the stream is re-scaled ONCE at the tower's output to
// put its largest element at ~2^13 (a power of two chosen on the device from the fp32 tensor: bit-repeatable), and every tower bucket is scaled back before it is
// reported.  amax_kernel: *bits = max |x| as float bits (atomicMax on non-negative floats' bit patterns is exact and order-independent).
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ in, long n4, unsigned* __restrict__ bits) {
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 v = *reinterpret_cast<const float4*>(in + i * 4);
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0.f && m <= 3.0e38f) atomicMax(bits, __float_as_uint(m));
}
// sc[0] = 2^k, sc[1] = 2^-k with k = clamp(floor(log2(target / amax)), 0, 24); bits is cleared for the next step
// target_mul (device, may be null): a power of two the target is multiplied by -- the step guard's delta, so that the stream follows the WHOLE loss scale
// 2^k delta as it follows fv_train_set_options' static one
__global__ void pick_scale_kernel(unsigned* __restrict__ bits, float* __restrict__ sc, float target, const float* __restrict__ target_mul) {
  if (target_mul) target *= *target_mul;
  const float amax = __uint_as_float(*bits);
  int k = 0;
  if (amax > 0.f) {
    k = (int)floorf(log2f(target / amax));
    k = k < 0 ? 0 : (k > 24 ? 24 : k);
  }
  sc[0] = ldexpf(1.0f, k);
  sc[1] = ldexpf(1.0f, -k);
  *bits = 0u;
}
__global__ __launch_bounds__(256) void scale_to_f16_dev_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, long n8, const float* __restrict__ sc, unsigned* sat) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const float scale = sc[0];
  const float4 a = *reinterpret_cast<const float4*>(in + i * 8), b = *reinterpret_cast<const float4*>(in + i * 8 + 4);
  float x[8] = {a.x * scale, a.y * scale, a.z * scale, a.w * scale, b.x * scale, b.y * scale, b.z * scale, b.w * scale};
  count_f16_sat8(x, sat);
  *reinterpret_cast<uint4*>(out + i * 8) = pack8_h(x);
}
__global__ __launch_bounds__(256) void scale_inplace_dev_kernel(float* __restrict__ p, long n4, const float* __restrict__ sc) {
  const float f = sc[1];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 v = *reinterpret_cast<float4*>(p + i * 4);
    v.x *= f; v.y *= f; v.z *= f; v.w *= f;
    *reinterpret_cast<float4*>(p + i * 4) = v;
  }
}

// layer-scaled 1x1 conv out = res + ls (.) (W h + b): from the UN-scaled products dWraw[c][j] = sum_m dout[m][c] h[m][j], dbraw[c] = sum_m dout[m][c]
//   dW[c][j] = ls[c] dWraw[c][j];  db[c] = ls[c] dbraw[c];  dls[c] = sum_j W[c][j] dWraw[c][j] + b[c] dbraw[c]      (one wave per output channel c)
__global__ __launch_bounds__(256) void ls_grads_kernel(const float* __restrict__ dWraw, const float* __restrict__ dbraw, const bf16_t* __restrict__ W,
                                                        const float* __restrict__ bias, const float* __restrict__ ls, float* __restrict__ dW,
                                                        float* __restrict__ db, float* __restrict__ dls, int C, int Kd) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float l = ls[c];
  float s = 0.f;
  for (int j = lane; j < Kd; j += 64) {
    const float r = dWraw[(size_t)c * Kd + j];
    s += bf2f(W[(size_t)c * Kd + j]) * r;
    dW[(size_t)c * Kd + j] = l * r;
  }
  s = wave_sum(s);
  if (lane == 0) {
    const float br = dbraw[c];
    db[c] = l * br;
    dls[c] = s + bias[c] * br;
  }
}

// ------------------------------------------------------------------------------------------------ LayerNormChannel backward
// y = w xhat + b, xhat = (x - mean) rstd over the C channels of a row.  dx (+ res) as fp16; per-block partial sums of dw = sum dy xhat, db = sum dy
// one wave per row, RPB rows per block (strided over its 4 waves); part[blk][2][C]
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, const float* __restrict__ w,
                                                      const bf16_t* __restrict__ res, bf16_t* __restrict__ dx, float* __restrict__ part, long rows, int C,
                                                      float eps, int rpb, unsigned* sat) {
  __shared__ float sred[4][2048];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nch = C >> 3;
  float aw[4][8], ab[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) { aw[i][e] = 0.f; ab[i][e] = 0.f; }
  const long r0 = (long)blockIdx.x * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
  for (long row = r0 + wv; row < r1; row += 4) {
    float v[4][8], g[4][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) {
        unpack8(*reinterpret_cast<const uint4*>(x + row * C + ch * 8), v[i]);
        unpack8_h(*reinterpret_cast<const uint4*>(dy + row * C + ch * 8), g[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[i][e];
      }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane + 64 * i < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; q += d * d; }
      }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xh = (v[i][e] - mean) * rstd;
          const float dyv = g[i][e];
          aw[i][e] += dyv * xh;
          ab[i][e] += dyv;
          const float gw = dyv * w[ch * 8 + e];
          v[i][e] = xh;
          g[i][e] = gw;
          s1 += gw;
          s2 += gw * xh;
        }
      }
    }
    s1 = wave_sum(s1) / (float)C;
    s2 = wave_sum(s2) / (float)C;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) {
        float o[8];
        if (res) unpack8_h(*reinterpret_cast<const uint4*>(res + row * C + ch * 8), o);
        else {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += rstd * (g[i][e] - s1 - v[i][e] * s2);
        count_f16_sat8(o, sat);
        *reinterpret_cast<uint4*>(dx + row * C + ch * 8) = pack8_h(o);
      }
    }
  }
  // fold the four waves (fixed order), dw then db
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = lane + 64 * i;
      if (ch < nch) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sred[wv][ch * 8 + e] = pass == 0 ? aw[i][e] : ab[i][e];
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) part[((size_t)blockIdx.x * 2 + pass) * C + c] = sred[0][c] + sred[1][c] + sred[2][c] + sred[3][c];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ tower attention backward (non-causal, head_dim 32)
// qkv bf16 [B*T][ld] = q | k | v (each C = heads * 32 wide, head h at column h * 32), dO fp16 [B*T][C] -> dqkv fp16 [B*T][ldd] in the
// same column order.  S = scale Q K^T, P = softmax(S), dV = P^T dO, dP = dO V^T, dS = P (dP - delta) scale, dQ = dS K, dK = dS^T Q.
// Both kernels keep the lane = query (dq) / key (dkv) layout of attention32_kernel: the score tile of a product over head_dim (its C/D registers) is the B
// operand of the following product over keys / queries, whose A operand (K^T, dO^T, Q^T) comes from the row-major LDS tile by ds_read_b64_tr_b16.
// Operands are converted to fp16 on the way into LDS / registers (bf16 widens exactly inside fp16's range); row statistics are recomputed here (log2
// domain), so neither forward kernel has to keep them and any token count works (keys / queries past T masked).
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
constexpr int TA_LD = 48;   // LDS row stride (halves) of a 32-wide tile: 96 B, 16-byte aligned rows for both the natural and the transposing reads

__device__ __forceinline__ uint4 bf8_to_h8(const uint4& u) {
  float f[8];
  unpack8(u, f);
  return pack8_h(f);
}
__device__ __forceinline__ f16x8 ta_tr_frag(const bf16_t* tile, int krow0, int dt, int fr) {
  // rows krow0 .. krow0 + 3 and 16 rows further, columns dt * 16 + 4 (fr & 3) .. + 3, through the transposing read: lane fr ends up with column
  // dt * 16 + fr of the eight rows {krow0 + j, krow0 + 16 + j}
  const bf16_t* vr = tile + (krow0 + (fr >> 2)) * TA_LD + dt * 16 + 4 * (fr & 3);
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(vr));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(vr + 16 * TA_LD));
  const uint2 lu = __builtin_bit_cast(uint2, lo), hu = __builtin_bit_cast(uint2, hi);
  return __builtin_bit_cast(f16x8, make_uint4(lu.x, lu.y, hu.x, hu.y));
}
__device__ __forceinline__ f16x8 ta_pack(const f32x4& a, const f32x4& b) {
  uint4 u;
  u.x = pack_h2(a[0], a[1]); u.y = pack_h2(a[2], a[3]); u.z = pack_h2(b[0], b[1]); u.w = pack_h2(b[2], b[3]);
  return __builtin_bit_cast(f16x8, u);
}
__device__ __forceinline__ float xor_sum_32_16(float v) { v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64); return v; }
__device__ __forceinline__ float xor_max_32_16b(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); v = fmaxf(v, __shfl_xor(v, 32, 64)); return v; }

struct TAttnParams {
  const bf16_t* qkv; const bf16_t* dO; bf16_t* dqkv; float* lse2; float* delta;
  int ld, lddo, ldd, B, T, heads, C; float scale;
};

// dQ (and the row statistics lse2 = log2 sum exp, delta = sum_d dO O): block = 64 queries of one (batch, head), lane = query
__global__ __launch_bounds__(256) void tattn_dq_kernel(TAttnParams p) {
  __shared__ __attribute__((aligned(16))) bf16_t sK[64 * TA_LD], sV[64 * TA_LD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int qblocks = (p.T + 63) >> 6;
  int bid = blockIdx.x;
  const int qb = bid % qblocks; bid /= qblocks;
  const int h = bid % p.heads;
  const int b = bid / p.heads;
  const int q = qb * 64 + wid * 16 + fr;
  const bool qok = q < p.T;
  const size_t qrow = (size_t)b * p.T + (qok ? q : 0);
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  const f16x8 fq = __builtin_bit_cast(f16x8, qok ? bf8_to_h8(*reinterpret_cast<const uint4*>(p.qkv + qrow * p.ld + h * 32 + fg * 8)) : zero4);
  const uint4 dou = qok ? *reinterpret_cast<const uint4*>(p.dO + qrow * p.lddo + h * 32 + fg * 8) : zero4;
  const f16x8 fdo = __builtin_bit_cast(f16x8, dou);
  const float c2 = p.scale * 1.4426950408889634f;
  const int nkb = (p.T + 63) >> 6;
  const int skey = tid >> 2, sch = tid & 3;
  const bf16_t* kbase = p.qkv + (size_t)b * p.T * p.ld + p.C + h * 32 + sch * 8;
  auto stage = [&](int kb, bool with_v) {
    const int key = kb * 64 + skey;
    const bool ok = key < p.T;
    const bf16_t* kp = kbase + (size_t)(ok ? key : 0) * p.ld;
    *reinterpret_cast<uint4*>(sK + skey * TA_LD + sch * 8) = ok ? bf8_to_h8(*reinterpret_cast<const uint4*>(kp)) : zero4;
    if (with_v) *reinterpret_cast<uint4*>(sV + skey * TA_LD + sch * 8) = ok ? bf8_to_h8(*reinterpret_cast<const uint4*>(kp + p.C)) : zero4;
  };
  // pass 1: running max / sum of the scaled scores (log2 domain) and delta = sum_j P_ij dP_ij from the SAME exponentials.  (The textbook shortcut
  // delta = sum_d dO O reads the forward's bf16-ROUNDED output: where the softmax is peaked, dP_ij - delta cancels and that 2^-9 shows up as 3e-3 in dQ / dK.)
  float m_run = -1e30f, l_run = 0.f, d_run = 0.f;
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    stage(kb, true);
    __syncthreads();
    f32x4 sacc[4], dacc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const f16x8 fk = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(sK + (kt * 16 + fr) * TA_LD + fg * 8));
      const f16x8 fv = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(sV + (kt * 16 + fr) * TA_LD + fg * 8));
      sacc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fk, fq, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      dacc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, fdo, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    float mloc = -1e30f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool kok = kb * 64 + kt * 16 + 4 * fg + r < p.T;
        sacc[kt][r] = kok ? sacc[kt][r] * c2 : -1e30f;
        mloc = fmaxf(mloc, sacc[kt][r]);
      }
    mloc = xor_max_32_16b(mloc);
    const float m_new = fmaxf(m_run, mloc);
    float ls = 0.f, ds = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(sacc[kt][r] - m_new);
        ls += e;
        ds += e * dacc[kt][r];
      }
    ls = xor_sum_32_16(ls);
    ds = xor_sum_32_16(ds);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    l_run = l_run * alpha + ls;
    d_run = d_run * alpha + ds;
    m_run = m_new;
  }
  const float lse2 = m_run + __builtin_amdgcn_logf(l_run);   // v_log_f32 is log2
  const float delta = d_run / l_run;
  if (qok && fg == 0) {
    p.lse2[((size_t)b * p.heads + h) * p.T + q] = lse2;
    p.delta[((size_t)b * p.heads + h) * p.T + q] = delta;
  }
  // pass 2: dQ^T += K^T dS^T
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    stage(kb, true);
    __syncthreads();
    f32x4 sacc[4], dacc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const f16x8 fk = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(sK + (kt * 16 + fr) * TA_LD + fg * 8));
      const f16x8 fv = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(sV + (kt * 16 + fr) * TA_LD + fg * 8));
      sacc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fk, fq, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      dacc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fv, fdo, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool kok = kb * 64 + kt * 16 + 4 * fg + r < p.T;
        const float pr = kok ? __builtin_amdgcn_exp2f(sacc[kt][r] * c2 - lse2) : 0.f;
        sacc[kt][r] = pr * (dacc[kt][r] - delta) * p.scale;
      }
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const f16x8 fp = ta_pack(sacc[2 * ks2], sacc[2 * ks2 + 1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ta_tr_frag(sK, (2 * ks2) * 16 + 4 * fg, dt, fr), fp, acc[dt], 0, 0, 0);
    }
  }
  if (qok) {
    bf16_t* op = p.dqkv + qrow * p.ldd + h * 32;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      uint2 u;
      u.x = pack_h2(acc[dt][0], acc[dt][1]);
      u.y = pack_h2(acc[dt][2], acc[dt][3]);
      *reinterpret_cast<uint2*>(op + dt * 16 + fg * 4) = u;
    }
  }
}

// dK, dV: block = 64 keys of one (batch, head), lane = key; Q and dO tiles (64 queries) row-major in LDS with their statistics
__global__ __launch_bounds__(256) void tattn_dkv_kernel(TAttnParams p) {
  __shared__ __attribute__((aligned(16))) bf16_t sQ[64 * TA_LD], sD[64 * TA_LD];
  __shared__ float sL[64], sDl[64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int kblocks = (p.T + 63) >> 6;
  int bid = blockIdx.x;
  const int kb = bid % kblocks; bid /= kblocks;
  const int h = bid % p.heads;
  const int b = bid / p.heads;
  const int key = kb * 64 + wid * 16 + fr;
  const bool kok = key < p.T;
  const size_t krow = (size_t)b * p.T + (kok ? key : 0);
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  const f16x8 fk = __builtin_bit_cast(f16x8, kok ? bf8_to_h8(*reinterpret_cast<const uint4*>(p.qkv + krow * p.ld + p.C + h * 32 + fg * 8)) : zero4);
  const f16x8 fv = __builtin_bit_cast(f16x8, kok ? bf8_to_h8(*reinterpret_cast<const uint4*>(p.qkv + krow * p.ld + 2 * p.C + h * 32 + fg * 8)) : zero4);
  const float c2 = p.scale * 1.4426950408889634f;
  const int nqb = (p.T + 63) >> 6;
  const int srow = tid >> 2, sch = tid & 3;
  f32x4 ak[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, av[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int qb = 0; qb < nqb; ++qb) {
    __syncthreads();
    {
      const int q = qb * 64 + srow;
      const bool ok = q < p.T;
      const size_t row = (size_t)b * p.T + (ok ? q : 0);
      *reinterpret_cast<uint4*>(sQ + srow * TA_LD + sch * 8) = ok ? bf8_to_h8(*reinterpret_cast<const uint4*>(p.qkv + row * p.ld + h * 32 + sch * 8)) : zero4;
      *reinterpret_cast<uint4*>(sD + srow * TA_LD + sch * 8) = ok ? *reinterpret_cast<const uint4*>(p.dO + row * p.lddo + h * 32 + sch * 8) : zero4;
      if (tid < 64) {
        const int q2 = qb * 64 + tid;
        const bool ok2 = q2 < p.T;
        sL[tid] = ok2 ? p.lse2[((size_t)b * p.heads + h) * p.T + q2] : 1e30f;   // exp2(s - 1e30) = 0: queries past T contribute nothing
        sDl[tid] = ok2 ? p.delta[((size_t)b * p.heads + h) * p.T + q2] : 0.f;
      }
    }
    __syncthreads();
    f32x4 sacc[4], dacc[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const f16x8 fq = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(sQ + (qt * 16 + fr) * TA_LD + fg * 8));
      const f16x8 fd = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(sD + (qt * 16 + fr) * TA_LD + fg * 8));
      sacc[qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fq, fk, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);    // rows = queries qt * 16 + 4 fg + r, column = this lane's key
      dacc[qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fd, fv, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    f32x4 pacc[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = qt * 16 + 4 * fg + r;
        const float pr = __builtin_amdgcn_exp2f(sacc[qt][r] * c2 - sL[qi]);
        pacc[qt][r] = pr;
        sacc[qt][r] = pr * (dacc[qt][r] - sDl[qi]) * p.scale;
      }
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const f16x8 fp = ta_pack(pacc[2 * ks2], pacc[2 * ks2 + 1]);
      const f16x8 fs = ta_pack(sacc[2 * ks2], sacc[2 * ks2 + 1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        av[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ta_tr_frag(sD, (2 * ks2) * 16 + 4 * fg, dt, fr), fp, av[dt], 0, 0, 0);
        ak[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ta_tr_frag(sQ, (2 * ks2) * 16 + 4 * fg, dt, fr), fs, ak[dt], 0, 0, 0);
      }
    }
  }
  if (kok) {
    bf16_t* kp = p.dqkv + krow * p.ldd + p.C + h * 32;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      uint2 u;
      u.x = pack_h2(ak[dt][0], ak[dt][1]); u.y = pack_h2(ak[dt][2], ak[dt][3]);
      *reinterpret_cast<uint2*>(kp + dt * 16 + fg * 4) = u;
      u.x = pack_h2(av[dt][0], av[dt][1]); u.y = pack_h2(av[dt][2], av[dt][3]);
      *reinterpret_cast<uint2*>(kp + p.C + dt * 16 + fg * 4) = u;
    }
  }
}

// ------------------------------------------------------------------------------------------------ conv_exp's SE + GELU, backward
// forward: s = mean_p e, r = relu(W1 s + b1), g = sigmoid(W2 r + b2), out = gelu(e g).   (e bf16 [B][P][C]; s, r, g kept by the forward)
// du = dout gelu'(e g) (fp16, written to `du`), dz2[b][c] = (sum_p du e) g (1 - g)
__global__ __launch_bounds__(256) void se_bwd_du_kernel(const bf16_t* __restrict__ e, const bf16_t* __restrict__ dout, const float* __restrict__ g,
                                                         bf16_t* __restrict__ du, float* __restrict__ dz2, int P, int C, unsigned* sat) {
  const int ch = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (ch >= (C >> 3)) return;
  float gv[8], a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 8; ++k) gv[k] = g[(size_t)b * C + ch * 8 + k];
  for (int p = 0; p < P; ++p) {
    const size_t off = ((size_t)b * P + p) * C + ch * 8;
    float ev[8], d[8];
    unpack8(*reinterpret_cast<const uint4*>(e + off), ev);
    unpack8_h(*reinterpret_cast<const uint4*>(dout + off), d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float gl, dg;
      gelu_and_grad(ev[k] * gv[k], gl, dg);
      d[k] *= dg;
      a[k] += d[k] * ev[k];
    }
    count_f16_sat8(d, sat);
    *reinterpret_cast<uint4*>(du + off) = pack8_h(d);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) dz2[(size_t)b * C + ch * 8 + k] = a[k] * gv[k] * (1.0f - gv[k]);
}
// y[b][n] = sum_k x[b][k] W[k * ldw + n], optionally masked by (gate[b][n] > 0).  Block = 16 outputs x 16 interleaved k classes (a thread per (b, n)
// walked K = 3072 dependent steps on 32 blocks: 0.9 ms of the step); the classes are added in order: bit-repeatable
__global__ __launch_bounds__(256) void matvec_t_kernel(const float* __restrict__ x, const float* __restrict__ W, int ldw, const float* __restrict__ gate,
                                                        float* __restrict__ y, int N, int K) {
  __shared__ float part[16][17];
  const int nl = threadIdx.x & 15, kc = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + nl, b = blockIdx.y;
  float s = 0.f;
  if (n < N)
    for (int k = kc; k < K; k += 16) s += x[(size_t)b * K + k] * W[(size_t)k * ldw + n];
  part[kc][nl] = s;
  __syncthreads();
  if (threadIdx.x < 16 && n < N) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += part[q][threadIdx.x];
    if (gate && !(gate[(size_t)b * N + n] > 0.f)) t = 0.f;
    y[(size_t)b * N + n] = t;
  }
}
// out[n][k] = sum_b a[b][n] v[b][k] (k < K), bias[n] = sum_b a[b][n]; thread per (n, k), k == K computes the bias
__global__ __launch_bounds__(256) void outer_sum_kernel(const float* __restrict__ a, const float* __restrict__ v, float* __restrict__ out, float* __restrict__ bias,
                                                         int B, int N, int K) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * (K + 1)) return;
  const int n = (int)(i / (K + 1)), k = (int)(i % (K + 1));
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += a[(size_t)b * N + n] * (k < K ? v[(size_t)b * K + k] : 1.0f);
  if (k < K) out[(size_t)n * K + k] = s;
  else bias[n] = s;
}
// de = du g + ds / P, in place over du (fp16)
__global__ __launch_bounds__(256) void se_bwd_de_kernel(bf16_t* __restrict__ du, const float* __restrict__ g, const float* __restrict__ ds, int P, int C,
                                                         long total_chunks, unsigned* sat) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total_chunks) return;
  const int nch = C >> 3;
  const int ch = (int)(i % nch);
  const long b = i / ((long)nch * P);
  float v[8];
  unpack8_h(*reinterpret_cast<const uint4*>(du + i * 8), v);
  const float invp = 1.0f / (float)P;
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = v[k] * g[b * C + ch * 8 + k] + ds[b * C + ch * 8 + k] * invp;
  count_f16_sat8(v, sat);
  *reinterpret_cast<uint4*>(du + i * 8) = pack8_h(v);
}

// ------------------------------------------------------------------------------------------------ stem conv 3x3 s2 (3 -> C0) + GELU, weight gradient
// a0 = b + sum_k w[k][co] patch[k] is recomputed from the pixels (B,S,S,4) bf16; da0 = dh0 gelu'(a0); dW[k][co] += da0 patch[k], db[co] += da0.
// thread = one output channel x a slice of the block's output pixels (the 27 patch values are a broadcast load); part[blk][28][C0]
__global__ __launch_bounds__(384) void stem0_wgrad_kernel(const bf16_t* __restrict__ pix, const float* __restrict__ w, const float* __restrict__ bias,
                                                           const bf16_t* __restrict__ dh0, float* __restrict__ part, int S, int C0, long npix, long ppb, int round_w) {
  extern __shared__ __attribute__((aligned(16))) float sr_st[];   // [NPS][28][C0]
  const int NPS = 384 / C0;
  const int co = threadIdx.x % C0, ps = threadIdx.x / C0;
  const int So = S >> 1;
  float wr[27], acc[28];
#pragma unroll
  for (int k = 0; k < 27; ++k) { const float wv = w[(size_t)k * C0 + co]; wr[k] = round_w ? bf2f(f2bf(wv)) : wv; }   // round_w: the forward's implicit-GEMM stem holds bf16 weights
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.f;
  const float bv = bias[co];
  if (ps < NPS) {
    // (ppb = rows per block here: the block walks whole output rows, its slices interleaved along a row -- no division per pixel)
    const long rows = npix / So, r0 = (long)blockIdx.x * ppb, r1 = r0 + ppb < rows ? r0 + ppb : rows;
    for (long row = r0; row < r1; ++row) {
      const int oy = (int)(row % So);
      const long b = row / So;
      for (int ox = ps; ox < So; ox += NPS) {
      const long p = row * So + ox;
      float pt[27];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - 1 + ky;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox * 2 - 1 + kx;
          float c0 = 0.f, c1 = 0.f, c2 = 0.f;
          if (iy >= 0 && iy < S && ix >= 0 && ix < S) {
            const uint2 u = *reinterpret_cast<const uint2*>(pix + ((b * S + iy) * S + ix) * 4);
            c0 = bf_lo(u.x); c1 = bf_hi(u.x); c2 = bf_lo(u.y);
          }
          pt[(ky * 3 + kx) * 3 + 0] = c0; pt[(ky * 3 + kx) * 3 + 1] = c1; pt[(ky * 3 + kx) * 3 + 2] = c2;
        }
      }
      float a0 = bv;
#pragma unroll
      for (int k = 0; k < 27; ++k) a0 += wr[k] * pt[k];
      f32x2 gl, dg2;
      gelu_and_grad2((f32x2){a0, 0.f}, gl, dg2);
      const _Float16 hv = __builtin_bit_cast(_Float16, dh0[p * C0 + co]);
      const float d = (float)hv * dg2.x;
#pragma unroll
      for (int k = 0; k < 27; ++k) acc[k] += d * pt[k];
      acc[27] += d;
      }
    }
  }
  if (ps < NPS) {
#pragma unroll
    for (int k = 0; k < 28; ++k) sr_st[(ps * 28 + k) * C0 + co] = acc[k];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 28 * C0; i += 384) {
    float s = 0.f;
    for (int q = 0; q < NPS; ++q) s += sr_st[(size_t)q * 28 * C0 + i];
    part[(size_t)blockIdx.x * 28 * C0 + i] = s;
  }
}

// The MFMA route to the same gradients (round 5, default where the GEMM kernels take the shapes): the 27-tap patches of every output pixel as fp16 rows
// P [B (S/2)^2][32] (column 27 = 1: the bias tap; 28 .. 31 = 0), so that a0 = P . [w | b]^T is an NT GEMM (FV_EPI_GELU_GRAD leaves gelu'(a0)) and
// [dW | db] = P^T . (dh0 gelu'(a0)) a TN GEMM over the pixels.  thread = one output pixel (64 bytes written)
__global__ __launch_bounds__(256) void stem_im2col16_kernel(const bf16_t* __restrict__ pix, bf16_t* __restrict__ P, int S, long npix) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const int So = S >> 1;
  const int ox = (int)(p % So);
  const long t = p / So;
  const int oy = (int)(t % So);
  const long b = t / So;
  float v[32];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * 2 - 1 + ky;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * 2 - 1 + kx;
      float c0 = 0.f, c1 = 0.f, c2 = 0.f;
      if (iy >= 0 && iy < S && ix >= 0 && ix < S) {
        const uint2 u = *reinterpret_cast<const uint2*>(pix + ((b * S + iy) * S + ix) * 4);
        c0 = bf_lo(u.x); c1 = bf_hi(u.x); c2 = bf_lo(u.y);
      }
      v[(ky * 3 + kx) * 3 + 0] = c0; v[(ky * 3 + kx) * 3 + 1] = c1; v[(ky * 3 + kx) * 3 + 2] = c2;
    }
  }
  v[27] = 1.0f; v[28] = v[29] = v[30] = v[31] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) *reinterpret_cast<uint4*>(P + p * 32 + q * 8) = pack8_h(v + q * 8);
}

// ------------------------------------------------------------------------------------------------ fv_train_commit, tower part
// one launch over a table of operations; a block takes 1024 consecutive destination elements of one operation
__global__ __launch_bounds__(256) void tower_commit_kernel(const TowerCommitOp* __restrict__ ops, int nops, const float* __restrict__ flat, unsigned* sat) {
  int lo = 0, hi = nops - 1;
  const int blk = blockIdx.x;
  while (lo < hi) {   // last op whose blk0 <= blk
    const int mid = (lo + hi + 1) >> 1;
    if (ops[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
  }
  const TowerCommitOp op = ops[lo];
  const long base = (long)(blk - op.blk0) * 1024;
  const float* src = flat + op.src_off;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long i = base + u * 256 + threadIdx.x;
    if (i >= op.n) return;
    switch (op.kind) {
      case 0: static_cast<float*>(op.dst)[i] = src[i]; break;
      case 1: static_cast<bf16_t*>(op.dst)[i] = f2bf(src[i]); break;
      case 2: {
        const int j = op.idx[i];
        static_cast<bf16_t*>(op.dst)[i] = j >= 0 ? f2bf(op.coef[i] * src[j]) : (bf16_t)0;
        break;
      }
      case 5: case 6: {   // packed image as fp16; 5: of the taps at the precision the forward holds them (bf16)
        const int j = op.idx[i];
        float v = j >= 0 ? op.coef[i] * src[j] : 0.f;
        if (op.kind == 5) v = bf2f(f2bf(v));
        static_cast<bf16_t*>(op.dst)[i] = __builtin_bit_cast(bf16_t, (_Float16)__builtin_amdgcn_fmed3f(v, -FV_F16_MAX, FV_F16_MAX));
        break;
      }
      default: {   // 3: dst f16 [cols][rows] = src[rows][cols]^T; 4: the same with row r of src scaled by flat[src2_off + r]
        const long j = i / op.rows, r = i % op.rows;
        float v = src[r * op.cols + j];
        if (op.kind == 4) v *= flat[op.src2_off + r];
        if (sat && !(fabsf(v) <= FV_F16_MAX)) atomicAdd(sat, 1u);
        v = __builtin_amdgcn_fmed3f(v, -FV_F16_MAX, FV_F16_MAX);
        static_cast<bf16_t*>(op.dst)[i] = __builtin_bit_cast(bf16_t, (_Float16)v);
      }
    }
  }
}

inline unsigned grid1(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }
inline unsigned gridr(long n) { return grid1(n, 64); }   // partial_reduce_kernel: 64 outputs per block

}  // namespace

// ================================================================================================ launchers
static int pick_slab(int C, int cap) {   // largest multiple of 8 that divides C and is <= cap
  int best = 8;
  for (int d = 8; d <= cap && d <= C; d += 8)
    if (C % d == 0) best = d;
  return best;
}

// row blocks of dw_wgrad_rows_kernel: enough blocks to fill the chip several times over (a block is 256 threads of ~170 registers: 2 .. 3 per CU), at least one
// output row per slice of a block
static int dw_wgrad_row_blocks(int nrows, int NPS, int nslabs) {
  int nrb = nrows / NPS;
  const int cap = 3072 / nslabs;
  if (nrb > cap) nrb = cap;
  return nrb < 1 ? 1 : nrb;
}
// blocks of dw_wgrad_lds_kernel: a group = NPS consecutive output rows of one image, gpb groups per block.  Two blocks are resident per CU (190 registers, 80 KB
// of LDS each): 512 blocks are ONE round of a 256-CU chip, and every block more is another partial-sum row for the reduce pass to read
struct DwWgLdsBlocks { int gpi, ngroups, gpb, nb; };
static DwWgLdsBlocks dw_wgrad_lds_blocks(int B, int Ho, int NPS, int nslabs) {
  DwWgLdsBlocks g;
  g.gpi = (Ho + NPS - 1) / NPS;
  g.ngroups = B * g.gpi;
  int nb = 512 / nslabs;
  if (nb < 1) nb = 1;
  if (nb > g.ngroups) nb = g.ngroups;
  g.gpb = (g.ngroups + nb - 1) / nb;
  g.nb = (g.ngroups + g.gpb - 1) / g.gpb;
  return g;
}
size_t dw_bwd_scratch_floats(int B, int Ho, int Wo, int Co, int k) {
  const long npix = (long)B * Ho * Wo;
  long npb = (npix + 255) / 256;
  if (npb > 512) npb = 512;
  const int CS = pick_slab(Co, 128);
  const long nrb = dw_wgrad_row_blocks(B * Ho, 256 / (CS / 2), Co / CS) + 1;
  // the LDS-staged form writes one row per block of row GROUPS, and groups do not cross images: B * ceil(Ho / NPS) of them can exceed B * Ho / NPS + 1
  // (B = 2, Ho = 9, NPS = 8: 4 against 3)
  const long nlds = dw_wgrad_lds_blocks(B, Ho, 256 / (CS / 2), Co / CS).nb;
  return (size_t)std::max(std::max(npb, nrb), nlds) * (k * k + 1) * Co;
}

// input gradient of a depthwise / channel-multiplier conv: dy fp16 (B,Ho,Wo,Ci*mult) -> dx fp16 (B,Hi,Wi,Ci) (+ res fp16); w fp32 tap-major [k*k][Ci*mult]
int launch_dw_dgrad(const bf16_t* dy, const float* w, const bf16_t* res, bf16_t* dx, int B, int Hi, int Wi, int Ci, int k, int stride, int mult, unsigned* sat,
                    hipStream_t s, int round_w) {
  if (!dy || !w || !dx) return fv_fail(FV_ERR_ARG, "dw_dgrad: null pointer");
  if (B <= 0 || Hi <= 0 || Wi <= 0 || Ci % 8) return fv_fail(FV_ERR_ARG, "dw_dgrad: bad shape C=%d", Ci);
  const int pad = k / 2;
  const int Ho = (Hi + 2 * pad - k) / stride + 1, Wo = (Wi + 2 * pad - k) / stride + 1;
  const int CS = pick_slab(Ci, mult == 1 ? 128 : 64);
  const int nslabs = Ci / CS, G = CS / 8, ppb = 256 / G, iters = 8;
  const long npix = (long)B * Hi * Wi;
  const long pblocks = (npix + (long)ppb * iters - 1) / ((long)ppb * iters);
  if (pblocks * nslabs > 0x7fffffffL) return fv_fail(FV_ERR_ARG, "dw_dgrad: grid too large");
  const dim3 grid((unsigned)(pblocks * nslabs));
  const size_t lds = (size_t)k * k * CS * mult * 4;
#define FV_DG(K_, S_, M_)                                                                                                              \
  if (k == K_ && stride == S_ && mult == M_) {                                                                                         \
    hipLaunchKernelGGL((dw_dgrad_kernel<K_, S_, M_>), grid, dim3(256), lds, s, dy, w, res, dx, Hi, Wi, Ci, Ho, Wo, CS, nslabs, npix, iters, sat, round_w); \
    FV_HIP_CHECK(hipGetLastError());                                                                                                   \
    return FV_OK;                                                                                                                      \
  }
  FV_DG(3, 1, 1) FV_DG(7, 1, 1) FV_DG(3, 2, 1) FV_DG(7, 2, 2) FV_DG(3, 1, 2)
#undef FV_DG
  return fv_fail(FV_ERR_UNSUPPORTED, "dw_dgrad: unsupported k=%d stride=%d mult=%d", k, stride, mult);
}

// tap + bias gradients: x bf16 (B,Hi,Wi,Ci), dy fp16 (B,Ho,Wo,Ci*mult) -> dw fp32 tap-major [k*k][Ci*mult], db [Ci*mult]; scratch >= dw_bwd_scratch_floats
int launch_dw_wgrad(const bf16_t* x, const bf16_t* dy, float* dw, float* db, float* scratch, int B, int Hi, int Wi, int Ci, int k, int stride, int mult,
                    hipStream_t s) {
  if (!x || !dy || !dw || !db || !scratch) return fv_fail(FV_ERR_ARG, "dw_wgrad: null pointer");
  const int Co = Ci * mult;
  if (B <= 0 || Hi <= 0 || Wi <= 0 || Co % 8) return fv_fail(FV_ERR_ARG, "dw_wgrad: bad shape C=%d", Ci);
  const int pad = k / 2;
  const int Ho = (Hi + 2 * pad - k) / stride + 1, Wo = (Wi + 2 * pad - k) / stride + 1;
  const int CS = pick_slab(Co, 128);
  const int nslabs = Co / CS, NPS = 256 / (CS / 2), NT = k * k + 1;
  // round 6: stride-1 maps of the RepMixer stages on the matrix cores (dw_wgrad_mfma_kernel): 32-column strips x 32-channel slices marching down the map
  static const bool no_wg_mfma = fv_ab_env("FASTVLA_NO_DW_WGRAD_MFMA") != nullptr;   // A/B (tools build)
  // (k = 7 only: measured per launch at C = 384, B = 32: 186 -> 98 us, against a ~80 us floor of its two input passes; the 3x3 instance is correct -- it stays compiled
  // for the tools build's FASTVLA_DW_WGRAD_MFMA3=1 -- but at 90 us it does not beat the VALU form's 88: both already sit at that floor)
  static const bool wg_mfma3 = fv_ab_env("FASTVLA_DW_WGRAD_MFMA3") != nullptr;
  if (!no_wg_mfma && (k == 7 || (k == 3 && wg_mfma3)) && stride == 1 && mult == 1 && Ci % 32 == 0 && Wi >= 32 && Hi >= 16 && (long)B * ((Wi + 31) / 32) <= 512 &&
      (size_t)B * Hi * Wi * Ci * 2 < ((size_t)1 << 40)) {
    const int tiles_x = (Wi + 31) / 32, nsl = Ci / 32;
    const long nb = (long)B * tiles_x, nstrips = nb * nsl;
    if (nstrips <= 0x7fffffffL && (size_t)nb * NT * Co <= dw_bwd_scratch_floats(B, Ho, Wo, Co, k)) {
      if (k == 7) {
        static bool attr7 = false;
        if (!attr7) { FV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dw_wgrad_mfma_kernel<7>), hipFuncAttributeMaxDynamicSharedMemorySize, DwWgGeo<7>::LDS)); attr7 = true; }
        hipLaunchKernelGGL((dw_wgrad_mfma_kernel<7>), dim3((unsigned)nstrips), dim3(256), (DwWgGeo<7>::LDS), s, x, dy, scratch, Hi, Wi, Ci, tiles_x, nsl);
      } else {
        static bool attr3 = false;
        if (!attr3) { FV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dw_wgrad_mfma_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, DwWgGeo<3>::LDS)); attr3 = true; }
        hipLaunchKernelGGL((dw_wgrad_mfma_kernel<3>), dim3((unsigned)nstrips), dim3(256), (DwWgGeo<3>::LDS), s, x, dy, scratch, Hi, Wi, Ci, tiles_x, nsl);
      }
      const long n = (long)NT * Co;
      hipLaunchKernelGGL(partial_reduce_kernel, dim3(gridr(n)), dim3(256), 0, s, scratch, nb, n, n, (long)k * k * Co, dw, db, 1.0f);
      FV_HIP_CHECK(hipGetLastError());
      return FV_OK;
    }
  }
  if ((k == 3 || k == 7) && Wo >= 8 && CS >= 32 * mult) {   // the LDS-staged form (dw_wgrad_lds_kernel)
    const int NPSl = 256 / (CS / 2);
    const DwWgLdsBlocks lb = dw_wgrad_lds_blocks(B, Ho, NPSl, nslabs);   // the same count dw_bwd_scratch_floats sized the scratch for
    const int gpi = lb.gpi, ngroups = lb.ngroups, gpb = lb.gpb, nb = lb.nb;
    const int NR = (NPSl - 1) * stride + k, NCc = 7 * stride + k;
    const size_t xb = (size_t)B * Hi * Wi * Ci * 2;
    if ((long)NR * NCc * (CS / mult / 8) <= 256L * 10 && xb < 0xfffffff0ull) {
      const size_t lds = 2 * 10 * 4096;   // two tiles of up to 10 x 256 16-byte pieces (>= the fold scratch: 10 x 256 x 2 floats)
      const dim3 grid((unsigned)(nb * nslabs));
#define FV_WL(K_, S_, M_)                                                                                                                                       \
  if (k == K_ && stride == S_ && mult == M_) {                                                                                                                  \
    static bool attr = false;                                                                                                                                   \
    if (!attr) {                                                                                                                                                \
      FV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dw_wgrad_lds_kernel<K_, S_, M_>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
      attr = true;                                                                                                                                              \
    }                                                                                                                                                           \
    hipLaunchKernelGGL((dw_wgrad_lds_kernel<K_, S_, M_>), grid, dim3(256), lds, s, x, dy, scratch, Hi, Wi, Co, CS, nslabs, ngroups, gpb, gpi, (unsigned)xb, Ho, Wo); \
    const long n = (long)NT * Co;                                                                                                                               \
    hipLaunchKernelGGL(partial_reduce_kernel, dim3(gridr(n)), dim3(256), 0, s, scratch, (long)nb, n, n, (long)k * k * Co, dw, db, 1.0f);                       \
    FV_HIP_CHECK(hipGetLastError());                                                                                                                            \
    return FV_OK;                                                                                                                                               \
  }
      FV_WL(3, 1, 1) FV_WL(7, 1, 1) FV_WL(3, 2, 1) FV_WL(7, 2, 2) FV_WL(3, 1, 2)
#undef FV_WL
    }
  }
  if ((k == 3 || k == 7) && Wo >= 8) {   // whole rows per thread (dw_wgrad_rows_kernel)
    const int nrows = B * Ho;
    const int nrb0 = dw_wgrad_row_blocks(nrows, NPS, nslabs);
    const int rpb = (nrows + nrb0 - 1) / nrb0;
    const int nrb = (nrows + rpb - 1) / rpb;
    const size_t lds = (size_t)10 * NPS * CS * 4;
    const dim3 grid((unsigned)(nrb * nslabs));
#define FV_WR(K_, S_, M_)                                                                                                                                  \
  if (k == K_ && stride == S_ && mult == M_) {                                                                                                             \
    hipLaunchKernelGGL((dw_wgrad_rows_kernel<K_, S_, M_>), grid, dim3(256), lds, s, x, dy, scratch, Hi, Wi, Co, CS, nslabs, nrows, rpb, Ho, Wo);           \
    const long n = (long)NT * Co;                                                                                                                          \
    hipLaunchKernelGGL(partial_reduce_kernel, dim3(gridr(n)), dim3(256), 0, s, scratch, (long)nrb, n, n, (long)k * k * Co, dw, db, 1.0f);                 \
    FV_HIP_CHECK(hipGetLastError());                                                                                                                       \
    return FV_OK;                                                                                                                                          \
  }
    FV_WR(3, 1, 1) FV_WR(7, 1, 1) FV_WR(3, 2, 1) FV_WR(7, 2, 2) FV_WR(3, 1, 2)
#undef FV_WR
  }
  const long npix = (long)B * Ho * Wo;
  long npb = (npix + 255) / 256;
  if (npb > 512) npb = 512;
  const long ppb = (npix + npb - 1) / npb;
  npb = (npix + ppb - 1) / ppb;
  const dim3 grid((unsigned)(npb * nslabs));
  const size_t lds = (size_t)10 * NPS * CS * 4;
#define FV_WG(K_, S_, M_)                                                                                                          \
  if (k == K_ && stride == S_ && mult == M_) {                                                                                     \
    hipLaunchKernelGGL((dw_wgrad_kernel<K_, S_, M_>), grid, dim3(256), lds, s, x, dy, scratch, Hi, Wi, Ci, Ho, Wo, CS, nslabs, npix, ppb); \
    const long n = (long)NT * Co;                                                                                                   \
    hipLaunchKernelGGL(partial_reduce_kernel, dim3(gridr(n)), dim3(256), 0, s, scratch, npb, n, n, (long)k * k * Co, dw, db, 1.0f); \
    FV_HIP_CHECK(hipGetLastError());                                                                                               \
    return FV_OK;                                                                                                                  \
  }
  FV_WG(3, 1, 1) FV_WG(7, 1, 1) FV_WG(3, 2, 1) FV_WG(7, 2, 2) FV_WG(3, 1, 2)
#undef FV_WG
  return fv_fail(FV_ERR_UNSUPPORTED, "dw_wgrad: unsupported k=%d stride=%d mult=%d", k, stride, mult);
}

// out[c] = sum_r in[r][c] over fp16 rows; scratch >= TOWER_COLSUM_CHUNKS * C floats
int launch_colsum16(const bf16_t* in, int ld, long R, int C, float* out, float* scratch, hipStream_t s) {
  if (!in || !out || !scratch || R <= 0 || C <= 0 || C % 8 || ld % 8) return fv_fail(FV_ERR_ARG, "colsum16: bad argument");
  long nch = (R + 63) / 64;
  if (nch > TOWER_COLSUM_CHUNKS) nch = TOWER_COLSUM_CHUNKS;
  const long rpc = (R + nch - 1) / nch;
  nch = (R + rpc - 1) / rpc;
  const int ncg = C >= 256 ? 32 : (C + 7) / 8;
  hipLaunchKernelGGL(colsum16_kernel, dim3((C + 255) / 256, (unsigned)nch), dim3(256), 0, s, in, ld, R, C, scratch, rpc, ncg);
  hipLaunchKernelGGL(partial_reduce_kernel, dim3(gridr(C)), dim3(256), 0, s, scratch, nch, (long)C, (long)C, (long)C, out, out, 1.0f);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_mul16(const bf16_t* a, const bf16_t* b, bf16_t* out, size_t n, unsigned* sat, hipStream_t s) {
  if (!a || !b || !out || n % 8) return fv_fail(FV_ERR_ARG, "mul16: bad argument");
  hipLaunchKernelGGL(mul16_kernel, dim3(grid1((long)(n / 8))), dim3(256), 0, s, a, b, out, (long)(n / 8), sat);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
int launch_gelu_grad_mul(const bf16_t* dh, const bf16_t* pre, bf16_t* out, size_t n, unsigned* sat, hipStream_t s) {
  if (!dh || !pre || !out || n % 8) return fv_fail(FV_ERR_ARG, "gelu_grad_mul: bad argument");
  hipLaunchKernelGGL(gelu_grad_mul_kernel, dim3(grid1((long)(n / 8))), dim3(256), 0, s, dh, pre, out, (long)(n / 8), sat);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
int launch_f16_to_f32(const bf16_t* in, float* out, size_t n, float scale, hipStream_t s) {
  if (!in || !out || n % 8) return fv_fail(FV_ERR_ARG, "f16_to_f32: bad argument");
  hipLaunchKernelGGL(f16_to_f32_kernel, dim3(grid1((long)(n / 8))), dim3(256), 0, s, in, out, (long)(n / 8), scale);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
int launch_scale_to_f16(const float* in, bf16_t* out, size_t n, float scale, unsigned* sat, hipStream_t s) {
  if (!in || !out || n % 8) return fv_fail(FV_ERR_ARG, "scale_to_f16: bad argument");
  hipLaunchKernelGGL(scale_to_f16_kernel, dim3(grid1((long)(n / 8))), dim3(256), 0, s, in, out, (long)(n / 8), scale, sat);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
// out f16 = in * 2^k with 2^k picked on the device so that max |in| 2^k ~ target (sc[0] = 2^k, sc[1] = 2^-k; bits: a zeroed device word of scratch)
int launch_rescale_to_f16(const float* in, bf16_t* out, size_t n, float target, unsigned* bits, float* sc, unsigned* sat, hipStream_t s, const float* target_mul_dev) {
  if (!in || !out || !bits || !sc || n % 8) return fv_fail(FV_ERR_ARG, "rescale_to_f16: bad argument");
  const long n4 = (long)(n / 4);
  hipLaunchKernelGGL(amax_kernel, dim3((unsigned)(n4 / 256 + 1 < 2048 ? n4 / 256 + 1 : 2048)), dim3(256), 0, s, in, n4, bits);
  hipLaunchKernelGGL(pick_scale_kernel, dim3(1), dim3(1), 0, s, bits, sc, target, target_mul_dev);
  hipLaunchKernelGGL(scale_to_f16_dev_kernel, dim3(grid1((long)(n / 8))), dim3(256), 0, s, in, out, (long)(n / 8), sc, sat);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
// p[0, n) *= sc[1] (n % 4 == 0, p 16-byte aligned)
int launch_unscale_dev(float* p, size_t n, const float* sc, hipStream_t s) {
  if (!p || !sc || n % 4 || ((uintptr_t)p & 15)) return fv_fail(FV_ERR_ARG, "unscale_dev: bad argument");
  const long n4 = (long)(n / 4);
  hipLaunchKernelGGL(scale_inplace_dev_kernel, dim3((unsigned)(n4 / 256 + 1 < 4096 ? n4 / 256 + 1 : 4096)), dim3(256), 0, s, p, n4, sc);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
int launch_ones_col(bf16_t* out, int ld, int C, long R, hipStream_t s) {
  if (!out || ld < C + 8 || ld % 8 || C % 8 || R <= 0) return fv_fail(FV_ERR_ARG, "ones_col: bad argument");
  hipLaunchKernelGGL(ones_col_kernel, dim3(grid1(R)), dim3(256), 0, s, out, ld, C, R);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}
int launch_ls_grads(const float* dWraw, const float* dbraw, const bf16_t* W, const float* bias, const float* ls, float* dW, float* db, float* dls, int C, int Kd,
                    hipStream_t s) {
  if (!dWraw || !dbraw || !W || !bias || !ls || !dW || !db || !dls) return fv_fail(FV_ERR_ARG, "ls_grads: null pointer");
  hipLaunchKernelGGL(ls_grads_kernel, dim3((C + 3) / 4), dim3(256), 0, s, dWraw, dbraw, W, bias, ls, dW, db, dls, C, Kd);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

size_t ln_bwd_scratch_floats(long rows, int C) {
  long nb = (rows + 15) / 16;
  if (nb > 512) nb = 512;
  return (size_t)nb * 2 * C;
}
int launch_ln_bwd(const bf16_t* x, const bf16_t* dy, const float* w, const bf16_t* res, bf16_t* dx, float* dw, float* db, float* scratch, long rows, int C,
                  float eps, unsigned* sat, hipStream_t s) {
  if (!x || !dy || !w || !dx || !dw || !db || !scratch) return fv_fail(FV_ERR_ARG, "ln_bwd: null pointer");
  if (rows <= 0 || C % 8 || C > 2048) return fv_fail(FV_ERR_ARG, "ln_bwd: bad shape rows=%ld C=%d", rows, C);
  long nb = (rows + 15) / 16;
  if (nb > 512) nb = 512;
  const int rpb = (int)((rows + nb - 1) / nb);
  nb = (rows + rpb - 1) / rpb;
  hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, s, x, dy, w, res, dx, scratch, rows, C, eps, rpb, sat);
  hipLaunchKernelGGL(partial_reduce_kernel, dim3(gridr(2L * C)), dim3(256), 0, s, scratch, nb, 2L * C, 2L * C, (long)C, dw, db, 1.0f);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

// stats: 2 * B * heads * T floats (lse2 | delta)
int launch_tower_attn_bwd(const bf16_t* qkv, int ld, const bf16_t* dO, int lddo, bf16_t* dqkv, int ldd, float* stats, int B, int T, int heads, float scale,
                          hipStream_t s) {
  if (!qkv || !dO || !dqkv || !stats) return fv_fail(FV_ERR_ARG, "tower_attn_bwd: null pointer");
  const int C = heads * 32;
  if (B <= 0 || T <= 0 || heads <= 0 || ld < 3 * C || lddo < C || ldd < 3 * C || (ld | lddo | ldd) % 8) return fv_fail(FV_ERR_ARG, "tower_attn_bwd: bad shape / strides");
  if (((uintptr_t)qkv | (uintptr_t)dO | (uintptr_t)dqkv) & 15) return fv_fail(FV_ERR_ARG, "tower_attn_bwd: misaligned pointer");
  TAttnParams p{qkv, dO, dqkv, stats, stats + (size_t)B * heads * T, ld, lddo, ldd, B, T, heads, C, scale};
  const long blocks = (long)B * heads * ((T + 63) / 64);
  if (blocks > 0x7fffffffL) return fv_fail(FV_ERR_ARG, "tower_attn_bwd: grid too large");
  hipLaunchKernelGGL(tattn_dq_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  hipLaunchKernelGGL(tattn_dkv_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

// conv_exp's SE + GELU backward.  e bf16 [B][P][C] (the depthwise conv's output), dout fp16 [B][P][C], se = the forward's scratch (s [B][C] | r [B][R] | g [B][C]);
// de fp16 [B][P][C] (the gradient the depthwise conv's backward continues from); dW1 [R][C], db1 [R], dW2 [C][R], db2 [C];
// tmp >= B * (2 C + 2 R) floats
int launch_se_bwd(const bf16_t* e, const bf16_t* dout, const float* se, const float* w1, const float* w2, bf16_t* de, float* dW1, float* db1, float* dW2,
                  float* db2, float* tmp, int B, int P, int C, int R, unsigned* sat, hipStream_t s) {
  if (!e || !dout || !se || !w1 || !w2 || !de || !dW1 || !db1 || !dW2 || !db2 || !tmp) return fv_fail(FV_ERR_ARG, "se_bwd: null pointer");
  if (B <= 0 || P <= 0 || C % 8 || R <= 0) return fv_fail(FV_ERR_ARG, "se_bwd: bad shape");
  const float* sp = se;
  const float* r = se + (size_t)B * C;
  const float* g = r + (size_t)B * R;
  float* dz2 = tmp;                       // [B][C]
  float* dz1 = dz2 + (size_t)B * C;       // [B][R]
  float* ds = dz1 + (size_t)B * R;        // [B][C]
  hipLaunchKernelGGL(se_bwd_du_kernel, dim3((C / 8 + 255) / 256, B), dim3(256), 0, s, e, dout, g, de, dz2, P, C, sat);
  // dr = W2^T dz2 (W2 [C][R]), masked by relu: dz1
  hipLaunchKernelGGL(matvec_t_kernel, dim3((R + 15) / 16, B), dim3(256), 0, s, dz2, w2, R, r, dz1, R, C);
  // ds = W1^T dz1 (W1 [R][C])
  hipLaunchKernelGGL(matvec_t_kernel, dim3((C + 15) / 16, B), dim3(256), 0, s, dz1, w1, C, static_cast<const float*>(nullptr), ds, C, R);
  hipLaunchKernelGGL(outer_sum_kernel, dim3(grid1((long)C * (R + 1))), dim3(256), 0, s, dz2, r, dW2, db2, B, C, R);
  hipLaunchKernelGGL(outer_sum_kernel, dim3(grid1((long)R * (C + 1))), dim3(256), 0, s, dz1, sp, dW1, db1, B, R, C);
  const long chunks = (long)B * P * (C / 8);
  hipLaunchKernelGGL(se_bwd_de_kernel, dim3(grid1(chunks)), dim3(256), 0, s, de, g, ds, P, C, chunks, sat);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

size_t stem0_wgrad_scratch_floats(int B, int S, int C0) {
  long nb = (long)B * (S / 2);
  if (nb > 1024) nb = 1024;
  return (size_t)nb * 28 * C0;
}
// pix bf16 (B,S,S,4), w fp32 [27][C0], dh0 fp16 (B,S/2,S/2,C0) = dL/d(gelu output) -> dw [27][C0], db [C0]
int launch_stem0_wgrad(const bf16_t* pix, const float* w, const float* bias, const bf16_t* dh0, float* dw, float* db, float* scratch, int B, int S, int C0,
                       hipStream_t s, int round_w) {
  if (!pix || !w || !bias || !dh0 || !dw || !db || !scratch) return fv_fail(FV_ERR_ARG, "stem0_wgrad: null pointer");
  if (B <= 0 || S < 2 || (S & 1) || C0 < 8 || C0 > 384) return fv_fail(FV_ERR_UNSUPPORTED, "stem0_wgrad: bad shape S=%d C0=%d", S, C0);
  const long npix = (long)B * (S / 2) * (S / 2), rows = (long)B * (S / 2);
  long nb = rows;
  if (nb > 1024) nb = 1024;
  const long ppb = (rows + nb - 1) / nb;   // rows per block
  nb = (rows + ppb - 1) / ppb;
  const int NPS = 384 / C0;
  hipLaunchKernelGGL(stem0_wgrad_kernel, dim3((unsigned)nb), dim3(384), (size_t)NPS * 28 * C0 * 4, s, pix, w, bias, dh0, scratch, S, C0, npix, ppb, round_w);
  const long n = 28L * C0;
  hipLaunchKernelGGL(partial_reduce_kernel, dim3(gridr(n)), dim3(256), 0, s, scratch, nb, n, n, 27L * C0, dw, db, 1.0f);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_stem_im2col16(const bf16_t* pix, bf16_t* P, int B, int S, hipStream_t s) {
  if (!pix || !P || B <= 0 || S < 2 || (S & 1)) return fv_fail(FV_ERR_ARG, "stem_im2col16: bad argument");
  const long npix = (long)B * (S / 2) * (S / 2);
  hipLaunchKernelGGL(stem_im2col16_kernel, dim3(grid1(npix)), dim3(256), 0, s, pix, P, S, npix);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

int launch_tower_commit(const TowerCommitOp* ops_dev, int nops, int nblocks, const float* flat, unsigned* sat, hipStream_t s) {
  if (!ops_dev || !flat || nops <= 0 || nblocks <= 0) return fv_fail(FV_ERR_ARG, "tower_commit: bad argument");
  hipLaunchKernelGGL(tower_commit_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, ops_dev, nops, flat, sat);
  FV_HIP_CHECK(hipGetLastError());
  return FV_OK;
}

}  // namespace fv
