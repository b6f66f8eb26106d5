// lora_direct_kernels.hip -- the DIRECT LoRA backward (fv_train_lora_forward_backward; host side csrc/lora_path.inc, csrc/train_path.inc).
//
// The projected mode forms the full weight gradient dW' = dY^T . X and projects it (lora_kernels.hip).  Here dA and dB of every adapted matrix come straight
// from the operands the one-pass fp16 backward holds when it reaches a packed tensor -- the gradient's fp16 rows dY [R][Np] and the kept activation X [R][K]
// (split bf16 [hi | lo], or fp16 rows for the SwiGLU output) -- and dW' is never formed:
//     P = dY . B   [R][r]        Q = X . A^T   [R][r]        dA = s . P^T . X   [r][K]        dB = s . dY^T . Q   [N][r]
// One call serves ONE packed tensor and every adapter inside it (q | k | v share X and the packed dqkv; gate and up share XN2 and the interleaved
// [8 gate | 8 up] columns): their P and Q sit side by side as the columns [slot * r, slot * r + r) of one [R][NCp] array, so
//   ldir_pq_kernel     reads dY once (P) and X once (Q);   ldir_outer_kernel   reads X once (dA) and dY once (dB)
// -- dY and X each leave HBM twice per packed tensor, whatever the number of adapters.  A packed tensor without a target gets no call.
// What is NOT read once: the small arrays.  P / Q ([R][NCp] fp32, 0.7 .. 7.9 MB at R = 10240) are re-read by every 32-column tile of X / dY in ldir_outer_kernel
// (28 .. 1184 times: from L2 / the memory-side cache at best), A and B by every 32-row block of ldir_pq_kernel; ldir_outer_kernel feeds one 2-byte element per
// lane and row to an MFMA step; and with only one of gate / up a target, the dB pass still computes the tiles of both halves of every 16-column group.  The
// kernels are the plain fp32 form -- chosen for the accuracy bar, not tuned for time (measured step times: DESIGN.md section 7).
//
// Arithmetic: v_mfma_f32_32x32x2_f32 throughout.  The operands are widened to fp32 as they are loaded (fp16 exactly; hi + lo of a split value exactly: the
// remainder's last bit is not below the fp32 value's it was cut from), A and B are read as fp32, P and Q are KEPT as fp32: NOTHING is rounded to 16 bits in
// these kernels, every product is an fp32 fma chain.  Summation order is fixed: ldir_pq_kernel cuts the contraction into PQ_WAVES ranges (one per wave) added in
// wave order; ldir_outer_kernel cuts the R rows into S ranges whose partial sums ldir_reduce_kernel adds in range order (no float atomics: two runs give the
// same bits).  Rows beyond R enter as zeros (R need not be a multiple of anything).
#include "kernels.h"

namespace fv {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ long long pick3(long long a, long long b, long long c, int i) { return i == 0 ? a : (i == 1 ? b : c); }

// which slot (adapter of this call; -1: none) a packed column of dY belongs to, and its logical row there (LoraMat's row map, inverted)
__device__ __forceinline__ int col_slot(const LoraDirectPack& pk, int c, int& i) {
  int part = 0;
  i = c;
  if (pk.kind == 1) {
    if (c >= pk.qd + pk.kd) { part = 2; i = c - pk.qd - pk.kd; }
    else if (c >= pk.qd) { part = 1; i = c - pk.qd; }
  } else if (pk.kind == 2) {
    part = (c >> 3) & 1;
    i = (c >> 4) * 8 + (c & 7);
  }
  return part == 0 ? pk.slot_of_part[0] : (part == 1 ? pk.slot_of_part[1] : pk.slot_of_part[2]);
}

// eight consecutive elements of an operand row as fp32.  XK 2: split bf16, value = p[c] + p[lo_off + c];  XK 3: fp16
template <int XK>
__device__ __forceinline__ void load_row8(const bf16_t* __restrict__ p, int lo_off, float* v) {
  if constexpr (XK == 3) {
    unpack8_h(*reinterpret_cast<const uint4*>(p), v);
  } else {
    float lo[8];
    unpack8(*reinterpret_cast<const uint4*>(p), v);
    unpack8(*reinterpret_cast<const uint4*>(p + lo_off), lo);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += lo[e];
  }
}
template <int XK>
__device__ __forceinline__ float load_elem(const bf16_t* __restrict__ p, int lo_off) {
  if constexpr (XK == 3) return (float)__builtin_bit_cast(_Float16, *p);
  else return bf2f(p[0]) + bf2f(p[lo_off]);
}

// SIDE 0: out = P [R][NCp] = dY . Bcat (src = dY, fp16 rows, contraction over the Np packed columns; Bcat[c][slot * r + j] = B_slot[i(c)][j] where column c
// belongs to slot, zero elsewhere).  SIDE 1: out = Q [R][NCp] = X . Acat^T (src = X, contraction over K; Acat = the slots' A stacked).
// Block = 32 rows; wave w takes the w-th of PQ_WAVES ranges of the contraction (in 16-element chunks: lane (lo, hi) loads 8 consecutive elements of row lo at chunk
// offset 8 hi, MFMA step e multiplies element e of both operands -- the contraction index is permuted the same way on both sides); the shares are
// added in wave order through LDS.  NT = NCp / 32 column tiles, all held by every wave.
constexpr int PQ_WAVES = 8;   // waves of a ldir_pq_kernel block = ranges of its contraction (the loop is bound by load latency: more waves, not more MFMA)
template <int XK, int NT, int SIDE>
__global__ __launch_bounds__(64 * PQ_WAVES) void ldir_pq_kernel(const LoraDirectPack pk, const bf16_t* __restrict__ src, int ld, int lo_off, int R,
                                                      const float* __restrict__ lora, float* __restrict__ out) {
  __shared__ float red[PQ_WAVES - 1][16 * 64];
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, lo = l & 31, hi = l >> 5;
  const int row = blockIdx.x * 32 + lo;
  const bool rok = row < R;
  const int r = pk.r, C = SIDE ? pk.K : pk.Np, nch = C / 16;
  const int ch0 = (int)((long)nch * w / PQ_WAVES), ch1 = (int)((long)nch * (w + 1) / PQ_WAVES);
  f32x16 acc[NT];
  int slot[NT], jj[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    const int j = t * 32 + lo;
    slot[t] = j / r;
    jj[t] = j - slot[t] * r;
    if (slot[t] >= pk.nm) slot[t] = -1;
  }
  const bf16_t* xrow = src + (size_t)(rok ? row : 0) * ld;
  for (int ch = ch0; ch < ch1; ++ch) {
    const int c = ch * 16 + hi * 8;
    float a[8];
    if constexpr (SIDE == 0) {
      int i0, iu;
      const int cs = col_slot(pk, c, i0);
      const int csu = col_slot(pk, ch * 16, iu);    // wave-uniform; for kind 0 / 1 the whole chunk lies in one part (parts start on multiples of 32)
      if (pk.kind != 2 && csu < 0) continue;        // columns of a matrix that is not a target: no work
      if (rok) load_row8<3>(xrow + c, 0, a);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (pk.kind != 2 && (csu * r > t * 32 + 31 || (csu + 1) * r <= t * 32)) continue;   // (wave-uniform) this tile holds no column of the chunk's slot
        const bool ok = slot[t] >= 0 && slot[t] == cs;
        const float* bp = lora + pick3(pk.b_off[0], pk.b_off[1], pk.b_off[2], ok ? cs : 0) + (size_t)(ok ? i0 : 0) * r + jj[t];
        float b[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) b[e] = ok ? bp[(size_t)e * r] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc[t], 0, 0, 0);
      }
    } else {
      if (rok) load_row8<XK>(xrow + c, lo_off, a);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const bool ok = slot[t] >= 0;
        const float* ap = lora + pick3(pk.a_off[0], pk.a_off[1], pk.a_off[2], ok ? slot[t] : 0) + (size_t)(ok ? jj[t] : 0) * pk.K + c;
        float b[8];
        if (ok) {
          const float4 u0 = *reinterpret_cast<const float4*>(ap), u1 = *reinterpret_cast<const float4*>(ap + 4);
          b[0] = u0.x; b[1] = u0.y; b[2] = u0.z; b[3] = u0.w; b[4] = u1.x; b[5] = u1.y; b[6] = u1.z; b[7] = u1.w;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) b[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (w > 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) red[w - 1][v * 64 + l] = acc[t][v];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float sum = acc[t][v];
#pragma unroll
        for (int k = 0; k < PQ_WAVES - 1; ++k) sum += red[k][v * 64 + l];
        const int orow = blockIdx.x * 32 + (v & 3) + 8 * (v >> 2) + 4 * hi;
        if (orow < R) out[(size_t)orow * pk.NCp + t * 32 + lo] = sum;
      }
    }
    __syncthreads();
  }
}

// part[s][j][u] = sum over the rows of range s of V[row][j] . U[row][u]: V = P or Q [R][NCp] (fp32), U = X (MODE 0: dA, u = input column) or dY (MODE 1: dB,
// u = packed output column).  Wave = one 32-column tile of U against all NT tiles of V; one MFMA step takes two rows (lane (lo, hi): row 2 step + hi,
// columns lo of both operands: coalesced row reads, no transposed copy of anything).  MODE 1 skips the V tiles that hold no column of the U tile's adapter
// (q | k | v: one slot per tile), and a U tile of a matrix without an adapter altogether.
template <int UK, int NT, int MODE>
__global__ __launch_bounds__(256) void ldir_outer_kernel(const LoraDirectPack pk, const bf16_t* __restrict__ U, int ldu, int lo_off, int Ucols,
                                                         const float* __restrict__ V, int R, int rpr, float* __restrict__ part) {
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, lo = l & 31, hi = l >> 5;
  const int u0 = (blockIdx.x * 4 + w) * 32;
  if (u0 >= Ucols) return;
  int t0 = 0, t1 = NT - 1;
  if (MODE == 1 && pk.kind != 2) {
    int iu;
    const int cs = col_slot(pk, u0, iu);
    if (cs < 0) return;
    t0 = cs * pk.r / 32;
    t1 = ((cs + 1) * pk.r - 1) / 32;
  }
  const int s = blockIdx.y, rbeg = s * rpr, rend = min(R, rbeg + rpr);
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
  const int NCp = pk.NCp;
  for (int rr = rbeg; rr < rend; rr += 8) {
    float a[4][NT], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = rr + 2 * q + hi;
      const bool ok = row < rend;
      b[q] = ok ? load_elem<UK>(U + (size_t)row * ldu + u0 + lo, lo_off) : 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) a[q][t] = (ok && t >= t0 && t <= t1) ? V[(size_t)row * NCp + t * 32 + lo] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t >= t0 && t <= t1) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][t], b[q], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t < t0 || t > t1) continue;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int j = t * 32 + (v & 3) + 8 * (v >> 2) + 4 * hi;
      part[((size_t)s * NCp + j) * Ucols + u0 + lo] = acc[t][v];
    }
  }
}

// MODE 0: dA_slot[j][k] = s . (range 0 + range 1 + ...) of part[.][slot * r + j][k];  MODE 1: dB_slot[i(c)][j] likewise from part[.][slot(c) * r + j][c]
template <int MODE>
__global__ __launch_bounds__(256) void ldir_reduce_kernel(const LoraDirectPack pk, const float* __restrict__ part, int S, int Ucols, float scale,
                                                          float* __restrict__ lgrads) {
  const int r = pk.r;
  const size_t n = (size_t)(MODE == 0 ? pk.nm * r : r) * Ucols, stride = (size_t)pk.NCp * Ucols;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const int row = (int)(e / Ucols), u = (int)(e - (size_t)row * Ucols);
    int j, slot, i = 0;
    if (MODE == 0) { j = row; slot = j / r; }
    else {
      slot = col_slot(pk, u, i);
      if (slot < 0) continue;
      j = slot * r + row;
    }
    const float* p = part + (size_t)j * Ucols + u;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += p[(size_t)s * stride];
    if (MODE == 0) lgrads[pick3(pk.a_off[0], pk.a_off[1], pk.a_off[2], slot) + (size_t)(j - slot * r) * Ucols + u] = scale * sum;
    else lgrads[pick3(pk.b_off[0], pk.b_off[1], pk.b_off[2], slot) + (size_t)i * r + row] = scale * sum;
  }
}

template <int XK, int NT, int SIDE>
void launch_pq(const LoraDirectPack& pk, const bf16_t* src, int ld, int lo_off, int R, const float* lora, float* out, hipStream_t s) {
  hipLaunchKernelGGL((ldir_pq_kernel<XK, NT, SIDE>), dim3((unsigned)((R + 31) / 32)), dim3(64 * PQ_WAVES), 0, s, pk, src, ld, lo_off, R, lora, out);
}
template <int UK, int NT, int MODE>
void launch_outer(const LoraDirectPack& pk, const bf16_t* U, int ldu, int lo_off, int Ucols, const float* V, int R, int rpr, int S, float* part, hipStream_t s) {
  hipLaunchKernelGGL((ldir_outer_kernel<UK, NT, MODE>), dim3((unsigned)((Ucols / 32 + 3) / 4), (unsigned)S), dim3(256), 0, s, pk, U, ldu, lo_off, Ucols, V, R, rpr,
                     part);
}

template <int NT>
void launch_all(const LoraDirectPack& pk, const bf16_t* dY, const bf16_t* X, int xkind, int ldx, int lo_off, int R, const float* lora, float* lgrads, float scale,
                float* P, float* Q, float* part, size_t part_floats, hipStream_t s) {
  launch_pq<3, NT, 0>(pk, dY, pk.Np, 0, R, lora, P, s);
  if (xkind == 3) launch_pq<3, NT, 1>(pk, X, ldx, 0, R, lora, Q, s);
  else launch_pq<2, NT, 1>(pk, X, ldx, lo_off, R, lora, Q, s);
  for (int mode = 0; mode < 2; ++mode) {
    const int Ucols = mode ? pk.Np : pk.K;
    // row ranges: enough waves to fill the chip, as many as the partial sums' room allows; whole 8-row rounds
    const int tiles = Ucols / 32;
    long S = std::max(1, std::min(64, 6144 / tiles));   // (about six waves per SIMD: the loop is bound by load latency, not by the matrix core)
    S = std::max<long>(1, std::min<long>(S, (long)(part_floats / ((size_t)pk.NCp * Ucols))));
    const int rpr = (int)(((R + S - 1) / S + 7) / 8 * 8);
    S = (R + rpr - 1) / rpr;
    if (mode == 0) {
      if (xkind == 3) launch_outer<3, NT, 0>(pk, X, ldx, 0, Ucols, P, R, rpr, (int)S, part, s);
      else launch_outer<2, NT, 0>(pk, X, ldx, lo_off, Ucols, P, R, rpr, (int)S, part, s);
      const size_t n = (size_t)pk.nm * pk.r * Ucols;
      hipLaunchKernelGGL(ldir_reduce_kernel<0>, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, pk, part, (int)S, Ucols, scale, lgrads);
    } else {
      launch_outer<3, NT, 1>(pk, dY, pk.Np, 0, Ucols, Q, R, rpr, (int)S, part, s);
      const size_t n = (size_t)pk.r * Ucols;
      hipLaunchKernelGGL(ldir_reduce_kernel<1>, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, pk, part, (int)S, Ucols, scale, lgrads);
    }
  }
}

}  // namespace

size_t lora_direct_scratch_floats(long R, int rank, int max_cols) {
  const size_t ncp = (size_t)(3 * rank + 31) / 32 * 32;
  return 2 * (size_t)R * ncp + std::max((size_t)8 << 20, ncp * (size_t)max_cols);   // P | Q | partial sums (32 MB, or one range of the widest tensor)
}

int launch_lora_direct(const LoraDirectPack& pk, const bf16_t* dY, const bf16_t* X, int xkind, int ldx, int lo_off, int R, const float* lora, float* lgrads,
                       float scale, float* scratch, size_t scratch_floats, hipStream_t s) {
  if (!dY || !X || !lora || !lgrads || !scratch || R <= 0) return fv_fail(FV_ERR_ARG, "lora_direct: null pointer or no rows");
  if (pk.r < 1 || pk.r > 64 || pk.nm < 1 || pk.nm > 3 || pk.kind < 0 || pk.kind > 2 || pk.NCp != (pk.nm * pk.r + 31) / 32 * 32)
    return fv_fail(FV_ERR_ARG, "lora_direct: bad pack (rank %d, %d adapters, kind %d, NCp %d)", pk.r, pk.nm, pk.kind, pk.NCp);
  if (pk.Np <= 0 || pk.K <= 0 || pk.Np % 32 || pk.K % 32 || (pk.kind == 1 && (pk.qd % 32 || pk.kd % 32 || pk.qd + 2 * pk.kd != pk.Np)))
    return fv_fail(FV_ERR_ARG, "lora_direct: packed tensor %d x %d (q %d, kv %d): dimensions must be multiples of 32", pk.Np, pk.K, pk.qd, pk.kd);
  if ((xkind != 2 && xkind != 3) || ldx % 8 || ldx < pk.K || (xkind == 2 && (lo_off % 8 || lo_off < pk.K || ldx < lo_off + pk.K)))
    return fv_fail(FV_ERR_ARG, "lora_direct: activation operand kind %d, row stride %d, lo offset %d for %d columns", xkind, ldx, lo_off, pk.K);
  for (int i = 0; i < pk.nm; ++i)
    if (pk.a_off[i] % 4 || pk.a_off[i] < 0 || pk.b_off[i] < 0) return fv_fail(FV_ERR_ARG, "lora_direct: adapter offsets must be non-negative (lora_A: multiples of 4 floats)");
  if (((uintptr_t)dY | (uintptr_t)X | (uintptr_t)lora | (uintptr_t)scratch) & 15) return fv_fail(FV_ERR_ARG, "lora_direct: buffers must be 16-byte aligned");
  const size_t pq = (size_t)R * pk.NCp;
  const size_t one = (size_t)pk.NCp * std::max(pk.Np, pk.K);
  if (scratch_floats < 2 * pq + one) return fv_fail(FV_ERR_STATE, "lora_direct: scratch too small (%zu floats, %zu needed)", scratch_floats, 2 * pq + one);
  float *P = scratch, *Q = scratch + pq, *part = scratch + 2 * pq;
  const size_t part_floats = scratch_floats - 2 * pq;
  switch (pk.NCp / 32) {
    case 1: launch_all<1>(pk, dY, X, xkind, ldx, lo_off, R, lora, lgrads, scale, P, Q, part, part_floats, s); break;
    case 2: launch_all<2>(pk, dY, X, xkind, ldx, lo_off, R, lora, lgrads, scale, P, Q, part, part_floats, s); break;
    case 3: launch_all<3>(pk, dY, X, xkind, ldx, lo_off, R, lora, lgrads, scale, P, Q, part, part_floats, s); break;
    case 4: launch_all<4>(pk, dY, X, xkind, ldx, lo_off, R, lora, lgrads, scale, P, Q, part, part_floats, s); break;
    case 5: launch_all<5>(pk, dY, X, xkind, ldx, lo_off, R, lora, lgrads, scale, P, Q, part, part_floats, s); break;
    default: launch_all<6>(pk, dY, X, xkind, ldx, lo_off, R, lora, lgrads, scale, P, Q, part, part_floats, s); break;
  }
  return hipGetLastError() == hipSuccess ? FV_OK : fv_fail(FV_ERR_HIP, "lora_direct: launch failed");
}

}  // namespace fv
