// lora_kernels.hip -- kernels of the LoRA mode of backbone training (fv_train_lora_*; host side csrc/lora_path.inc).
//
// Every adapted decoder matrix runs as W' = W0 + s . B . A (A [r][in], B [out][r], s = alpha / r; PEFT's merged LoRA without dropout): the commit
// evaluates W' in fp32 and rounds it into the operand images the existing kernels read, so forward, backward and inference need nothing new, and
// the backward's full weight gradient dW' (fp32, flat_grads) is PROJECTED onto the adapters:
//     dA = s . B^T . dW'          dB = s . dW' . A^T
// Three kernels, all on the f32-input matrix core (v_mfma_f32_32x32x2_f32: exact fp32, bitwise an fmaf chain):
//   lora_project_kernel   one pass over dW' (ranks above 32: two): a wave loads a 32 x 32 tile once, uses it as loaded for dA and, transposed through LDS,
//                         for dB; dB leaves complete per 128-row strip, dA as per-strip partial sums that lora_reduce_kernel adds in strip order (no float
//                         atomics: the gradients are bit-reproducible, as everywhere in this library)
//   lora_commit_kernel<0> commit_kernel's matrix path (train_kernels.hip) with W0 + s . B . A in place of W0: the 64 x 64 tile of B . A first, into LDS
//   lora_commit_kernel<1> the same fp32 values written back into a flat master (fv_train_lora_merge): ONE device function, one summation order
// The adapters belong to LOGICAL matrices (q, k, v, o, gate, up, down), the gradient and the master are in the library's packed layouts: LoraMat
// carries the row map (logical row i sits in packed row row0 + (i >> 3) * blk + (i & 7): blk = 8 plain / q|k|v ranges, 16 gate / up interleaved).
//
// DoRA (the DORA = 1 instances; PEFT's use_dora): W' = diag(c) . V, V = W0 + s . B . A, c_i = m_i / n_i, n_i = ||V_i,:||_2 held constant in the backward,
// m a trained magnitude per output row.  lora_norm_kernel evaluates n (and, on request, m <- n) with the commit's own V; the commit multiplies each row by c_i
// before it rounds; the projection leaves  dA = s . B^T . diag(c) . dW',  dB = s . diag(c) . dW' . A^T  and
//     dm_i = (sum_j dW'_ij . V_ij) / n_i = (sum_j dW'_ij . W0_ij + s . sum_k B_ik . (dW' . A^T)_ik) / n_i
// -- one more fp32 stream (the master's rows of W0) beside dW'; the second term is the dB accumulator the wave already holds.  c enters the dA contraction on
// the B^T operand (c_i . B_ik, scaled once per strip) and dB on the way out (c_i . accB_ik): the walk over dW' multiplies nothing extra.
#include "kernels.h"

namespace fv {
namespace {

constexpr int TP = 64;        // commit tile (as commit_kernel)
constexpr int LSTRIP = LORA_STRIP_ROWS;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void load8(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// One launch covers the adapter rows [k0, k0 + 32) (ranks above 32 take a second launch, which reads dW' again).  Block = one strip of <= 128 logical rows of
// one matrix, wave w = its rows [32 w, 32 w + 32); the block walks the 32-column blocks together.  Per column block each wave loads its 32 x 32 tile of dW'
// once (coalesced rows), uses it as loaded for dA (contraction over rows) and through LDS, transposed, for dB (contraction over columns).  dB stays in the
// wave's accumulator over the whole walk and leaves complete; dA's four per-wave shares are added in wave order and leave as the strip's partial sum.
// DORA: see the head of this file.  dm's W0 stream is read by the k0 = 0 launch only; a second launch (ranks above 32) adds its share of the B term to the dm
// the first one stored (same stream, one owner thread per row: no atomics), so W0 is streamed once and dm is complete after the last launch.
template <int DORA>
__global__ __launch_bounds__(256) void lora_project_kernel(const LoraMat* __restrict__ mats, int m0, int m1, int strip_begin, const float* __restrict__ g,
                                                            const float* __restrict__ lora, float* __restrict__ lgrads, float* __restrict__ part, int r, int k0,
                                                            float scale, const float* __restrict__ master, const float* __restrict__ norms) {
  __shared__ float T[4][32 * 33];    // per wave: its tile of dW' (row stride 33: the transposed read is conflict-free)
  __shared__ float As[32 * 33];      // A[k0 .. k0 + 32)[j0 .. j0 + 32), zeros beyond the rank
  __shared__ float red[4][16 * 64];  // the waves' dA shares of this column block
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lo = l & 31, hi = l >> 5;
  const int strip = strip_begin + blockIdx.x;
  int a = m0, b = m1 - 1;          // the last matrix whose strip0 <= strip
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (mats[mid].strip0 <= strip) a = mid; else b = mid - 1;
  }
  const LoraMat d = mats[a];
  const int ls = strip - d.strip0, i0 = ls * LSTRIP + 32 * w;
  const bool valid = i0 < d.out;     // (wave-uniform: a matrix's last strip may hold fewer than four row tiles)
  const int in = d.in, ncb = in / 32;
  const float* W = g + d.w_off;
  const float* A = lora + d.a_off;
  const float* Bm = lora + d.b_off;
  float* P = part + d.part_off + (size_t)ls * r * in;
  float* Tw = T[w];
  // B^T operand of this wave's rows: lane (lo, hi) holds B[i0 + 2 v + hi][k0 + lo]; the rows' packed positions in dW'
  float bB[16];
  size_t wrow[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = i0 + 2 * v + hi;
    bB[v] = (valid && k0 + lo < r) ? Bm[(size_t)i * r + k0 + lo] : 0.f;
    wrow[v] = (size_t)(d.row0 + (i >> 3) * d.blk + (i & 7)) * in;
    if constexpr (DORA) {
      if (valid) bB[v] *= lora[d.m_off + i] / norms[d.n_off + i];     // c_i . B[i][k]
    }
  }
  f32x16 accB;
#pragma unroll
  for (int v = 0; v < 16; ++v) accB[v] = 0.f;

  // (the next column block's tile and A rows are fetched into registers while this one is being multiplied: the loads' latency hides under 32 MFMAs)
  float xn[16], an[4];
#pragma unroll
  for (int v = 0; v < 16; ++v) xn[v] = valid ? W[wrow[v] + lo] : 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = k0 + (tid >> 5) + 8 * q;
    an[q] = k < r ? A[(size_t)k * in + lo] : 0.f;
  }
  // DoRA: the master's tile of W0 travels beside dW' (same packed rows, same prefetch); gw[v] = this lane's share of sum_j dW'[i][j] . W0[i][j], i = 2 v + hi
  const float* W0 = DORA ? master + d.w_off : nullptr;
  const bool dot = DORA && valid && k0 == 0;
  float gw[DORA ? 16 : 1], wn[DORA ? 16 : 1];
  if constexpr (DORA) {
#pragma unroll
    for (int v = 0; v < 16; ++v) { gw[v] = 0.f; wn[v] = dot ? W0[wrow[v] + lo] : 0.f; }
  }
  for (int cb = 0; cb < ncb; ++cb) {
    const int j0 = cb * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) As[((tid >> 5) + 8 * q) * 33 + lo] = an[q];
    f32x16 accA;
#pragma unroll
    for (int v = 0; v < 16; ++v) accA[v] = 0.f;
    float x[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) x[v] = xn[v];
    float w0[DORA ? 16 : 1];
    if constexpr (DORA) {
#pragma unroll
      for (int v = 0; v < 16; ++v) w0[v] = wn[v];
      if (cb + 1 < ncb && dot) {
#pragma unroll
        for (int v = 0; v < 16; ++v) wn[v] = W0[wrow[v] + j0 + 32 + lo];
      }
    }
    if (cb + 1 < ncb) {
#pragma unroll
      for (int v = 0; v < 16; ++v) xn[v] = valid ? W[wrow[v] + j0 + 32 + lo] : 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + (tid >> 5) + 8 * q;
        an[q] = k < r ? A[(size_t)k * in + j0 + 32 + lo] : 0.f;
      }
    }
    if (valid) {
#pragma unroll
      for (int v = 0; v < 16; ++v) Tw[(2 * v + hi) * 33 + lo] = x[v];
      // dA[k][j] += sum_i B[i][k] . dW'[i][j]:  a = B^T (lane: k = lo, i = 2 v + hi), b = dW' rows as loaded
#pragma unroll
      for (int v = 0; v < 16; ++v) accA = __builtin_amdgcn_mfma_f32_32x32x2f32(bB[v], x[v], accA, 0, 0, 0);
      if constexpr (DORA) {
#pragma unroll
        for (int v = 0; v < 16; ++v) gw[v] = fmaf(x[v], w0[v], gw[v]);
      }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) red[w][v * 64 + l] = accA[v];
    __syncthreads();
    if (valid) {
      // dB[i][k] += sum_j dW'[i][j] . A[k][j]:  a = dW' (lane: i = lo, j = 2 u + hi: the transposed read), b = A^T (lane: k = lo, j = 2 u + hi)
#pragma unroll
      for (int u = 0; u < 16; ++u) accB = __builtin_amdgcn_mfma_f32_32x32x2f32(Tw[lo * 33 + 2 * u + hi], As[lo * 33 + 2 * u + hi], accB, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q, v = e >> 6, ll = e & 63;
      const float sum = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
      const int k = k0 + (v & 3) + 8 * (v >> 2) + 4 * (ll >> 5);
      if (k < r) P[(size_t)k * in + j0 + (ll & 31)] = sum;
    }
    __syncthreads();
  }
  if (valid) {
    float* dB = lgrads + d.b_off;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = (v & 3) + 8 * (v >> 2) + 4 * hi;
      if constexpr (DORA) {
        if (k0 + lo < r) dB[(size_t)(i0 + row) * r + k0 + lo] = scale * (lora[d.m_off + i0 + row] / norms[d.n_off + i0 + row]) * accB[v];
      } else {
        if (k0 + lo < r) dB[(size_t)(i0 + row) * r + k0 + lo] = scale * accB[v];
      }
    }
  }
  if constexpr (DORA) {
    // dm: both row sums are 32 lane-partial sums (lane lo: its columns / its k), combined in a fixed butterfly, then through LDS (T is free: the walk ended on
    // a barrier) into one thread per row
    if (valid) {
      float bt[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = (v & 3) + 8 * (v >> 2) + 4 * hi;
        bt[v] = k0 + lo < r ? Bm[(size_t)(i0 + row) * r + k0 + lo] * accB[v] : 0.f;
      }
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          bt[v] += __shfl_xor(bt[v], off);
          gw[v] += __shfl_xor(gw[v], off);
        }
      }
      if (lo == 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          Tw[2 * v + hi] = gw[v];
          Tw[32 + (v & 3) + 8 * (v >> 2) + 4 * hi] = bt[v];
        }
      }
    }
    __syncthreads();
    if (valid && l < 32) {
      const float n = norms[d.n_off + i0 + l];
      float* dm = lgrads + d.m_off + i0 + l;
      if (k0 == 0) *dm = (Tw[l] + scale * Tw[32 + l]) / n;
      else *dm += scale * Tw[32 + l] / n;
    }
  }
}

// dA[k][j] = s . (strip 0 + strip 1 + ...), one thread per element, blockIdx.y = matrix
__global__ __launch_bounds__(256) void lora_reduce_kernel(const LoraMat* __restrict__ mats, int m0, const float* __restrict__ part, float* __restrict__ lgrads,
                                                           int r, float scale) {
  const LoraMat d = mats[m0 + blockIdx.y];
  const size_t n = (size_t)r * d.in;
  const int ns = (d.out + LSTRIP - 1) / LSTRIP;
  const float* P = part + d.part_off;
  float* dA = lgrads + d.a_off;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    float sum = 0.f;
    for (int s = 0; s < ns; ++s) sum += P[(size_t)s * n + e];
    dA[e] = scale * sum;
  }
}

// which adapter a packed row belongs to (-1: none) and its logical row there
__device__ __forceinline__ int lora_row_mat(const LoraCommitDesc& d, int prow, int& i) {
  int part = 0;
  i = prow;
  if (d.kind == 1) {
    if (prow >= d.qd + d.kd) { part = 2; i = prow - d.qd - d.kd; }
    else if (prow >= d.qd) { part = 1; i = prow - d.qd; }
  } else if (d.kind == 2) {
    part = (prow >> 3) & 1;
    i = (prow >> 4) * 8 + (prow & 7);
  }
  return part == 0 ? d.mat[0] : (part == 1 ? d.mat[1] : d.mat[2]);
}

// The ONE place B . A is evaluated (commit and merge both call it): the 64 x 64 tile (r0, c0) of sum_k B[i][k] . A[k][j] into `tile`, on v_mfma_f32_32x32x2_f32
// (exact fp32, k ascending).  Wave w takes the 32 x 32 quarter (w >> 1, w & 1).  Rows of one tile may belong to two adapters (gate / up interleaved by 8):
// one pass per adapter, the rows of the other entering as zeros; rows without an adapter get zeros.
__device__ __forceinline__ void lora_delta_tile(const LoraCommitDesc& d, const LoraMat* __restrict__ mats, int r0, int c0, const float* __restrict__ lora, int r,
                                                float (*tile)[TP + 1]) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lo = l & 31, hi = l >> 5;
  const int prow = r0 + 32 * (w >> 1) + lo, col = c0 + 32 * (w & 1) + lo;
  int i = 0;
  const int mine = prow < d.c.rows ? lora_row_mat(d, prow, i) : -1;
  f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  const int npass = d.kind == 2 ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    // the adapter of this pass: tile-uniform (q | k | v ranges start on multiples of 64 rows: the tile's first row decides)
    int i_unused;
    const int mi = d.kind == 2 ? (pass == 0 ? d.mat[0] : d.mat[1]) : lora_row_mat(d, r0, i_unused);
    if (mi < 0) continue;
    const LoraMat m = mats[mi];
    const float* A = lora + m.a_off;
    const float* Bm = lora + m.b_off + (size_t)i * r;
    const bool rowok = mine == mi, colok = col < d.c.cols;
    for (int k = 0; k < r; k += 8) {     // four k-pairs per round: their eight loads are in flight together (k >= rank enters as zeros)
      float av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int kk = k + 2 * q + hi;
        av[q] = (rowok && kk < r) ? Bm[kk] : 0.f;
        bv[q] = (colok && kk < r) ? A[(size_t)kk * m.in + col] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[q], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int v = 0; v < 16; ++v) tile[32 * (w >> 1) + (v & 3) + 8 * (v >> 2) + 4 * hi][32 * (w & 1) + lo] = acc[v];
}

// DoRA's row norms: n_i = ||V_i,:||_2, V = W0 + s . B . A exactly as the commit below evaluates it (the same device function, the same fmaf).  Block = one
// 64-row band of one packed tensor, walking its 64-column tiles; per row eight lanes each keep a partial sum of squares over their 8 columns of every tile
// (the 8 squares of a tile added as a tree first), combined at the end in a fixed butterfly: 8 lane-partial sums of in / 64 terms, not one running sum of `in`.
// (A band whose rows carry no adapter -- the k rows when only q and v are targets -- is walked all the same and writes nothing: wasted reads, correct result.)
// mag non-null: the magnitudes of that trainable buffer receive the same values (fv_train_lora_init_magnitude: c = m / n is then exactly 1).
__global__ __launch_bounds__(256) void lora_norm_kernel(const LoraCommitDesc* __restrict__ desc, int ndesc, const LoraMat* __restrict__ mats,
                                                         const float* __restrict__ flat, const float* __restrict__ lora, int r, float scale,
                                                         float* __restrict__ norms, float* __restrict__ mag) {
  __shared__ float tile[TP][TP + 1];
  const int tid = threadIdx.x, bb = blockIdx.x;
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].band0 <= bb) lo = mid; else hi = mid - 1;
  }
  const LoraCommitDesc ld = desc[lo];
  const CommitDesc& d = ld.c;
  const float* src = flat + d.src_off;
  const int r0 = (bb - ld.band0) * TP, tcols = (d.cols + TP - 1) / TP;
  float acc[2] = {0.f, 0.f};
  for (int ct = 0; ct < tcols; ++ct) {
    const int c0 = ct * TP;
    lora_delta_tile(ld, mats, r0, c0, lora, r, tile);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int rr = (tid >> 3) + 32 * k, c = (tid & 7) * 8;
      if (r0 + rr < d.rows && c0 + c < d.cols) {
        float v[8];
        load8(src + (size_t)(r0 + rr) * d.cols + c0 + c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = fmaf(scale, tile[rr][c + e], v[e]);
          v[e] *= v[e];
        }
        acc[k] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float a = acc[k];
    a += __shfl_xor(a, 1);
    a += __shfl_xor(a, 2);
    a += __shfl_xor(a, 4);
    const int prow = r0 + (tid >> 3) + 32 * k;
    if ((tid & 7) == 0 && prow < d.rows) {
      int i = 0;
      const int mi = lora_row_mat(ld, prow, i);
      if (mi >= 0) {
        const float n = sqrtf(a);
        norms[mats[mi].n_off + i] = n;
        if (mag) mag[mats[mi].m_off + i] = n;
      }
    }
  }
}

// MERGE = 0: the operand images of the adapted tensors (bf16 rows, the active transposed copy, the fp16 row copy of the one-pass fp16 training forward) from
// W0 + s . B . A -- tile for tile what commit_kernel does with W0.  MERGE = 1: the fp32 values themselves, back into the master.
// DORA = 1: every row times c_i = m_i / n_i (norms as lora_norm_kernel left them) before anything is rounded or written; c_i == 1.0f leaves the bits alone.
// (n_i is not guarded against 0: an all-zero row of W0 + s . B . A gives 0 / 0 = NaN here, in the merge and in the projection, as in PEFT; trained weights
// have no such row.)
template <int MERGE, int DORA>
__global__ __launch_bounds__(256) void lora_commit_kernel(const LoraCommitDesc* __restrict__ desc, int ndesc, const LoraMat* __restrict__ mats, float* flat,
                                                           const float* __restrict__ lora, int r, float scale, int f16t, unsigned* __restrict__ sat,
                                                           const float* __restrict__ norms) {
  __shared__ float tile[TP][TP + 1];
  const int tid = threadIdx.x, bt = blockIdx.x;
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].c.tile0 <= bt) lo = mid; else hi = mid - 1;
  }
  const LoraCommitDesc ld = desc[lo];
  const CommitDesc& d = ld.c;
  const int lt = bt - d.tile0;
  float* src = flat + d.src_off;
  const int tcols = (d.cols + TP - 1) / TP;
  const int r0 = (lt / tcols) * TP, c0 = (lt % tcols) * TP;
  bf16_t* dst = static_cast<bf16_t*>(d.dst);
  const bool tr = !MERGE && d.dstT16 != nullptr;
  lora_delta_tile(ld, mats, r0, c0, lora, r, tile);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int rr = (tid >> 3) + 32 * k, c = (tid & 7) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r0 + rr < d.rows && c0 + c < d.cols) {
      load8(src + (size_t)(r0 + rr) * d.cols + c0 + c, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaf(scale, tile[rr][c + e], v[e]);    // W0 + s . (B . A); each thread reads, then reuses, its own 8 slots of the tile
      if constexpr (DORA) {
        int i = 0;
        const int mi = lora_row_mat(ld, r0 + rr, i);
        if (mi >= 0) {
          const float cr = lora[mats[mi].m_off + i] / norms[mats[mi].n_off + i];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] *= cr;
        }
      }
      if constexpr (MERGE) {
        store8(src + (size_t)(r0 + rr) * d.cols + c0 + c, v);
      } else {
        const uint4 hv = pack8(v);
        *reinterpret_cast<uint4*>(dst + (size_t)(r0 + rr) * d.cols + c0 + c) = hv;
        unpack8(hv, v);   // the transposed copy holds the ROUNDED weight (what the forward multiplies by)
        if (d.dst16) {
          float w16[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) w16[e] = v[e] * d.scale16;
          count_f16_sat8(w16, sat);
          *reinterpret_cast<uint4*>(static_cast<bf16_t*>(d.dst16) + (size_t)(r0 + rr) * d.cols + c0 + c) = pack8_h(w16);
        }
      }
    }
    if (tr) {
#pragma unroll
      for (int e = 0; e < 8; ++e) tile[rr][c + e] = v[e];
    }
  }
  if (!tr) return;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = (tid >> 3) + 32 * k, rr = (tid & 7) * 8;
    if (c0 + c >= d.cols || r0 + rr >= d.rows) continue;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[rr + e][c];
    if (f16t) {
      count_f16_sat8(v, sat);
      *reinterpret_cast<uint4*>(static_cast<bf16_t*>(d.dstT16) + (size_t)(c0 + c) * d.rows + r0 + rr) = pack8_h(v);
    } else {
      *reinterpret_cast<uint4*>(static_cast<bf16_t*>(d.dstTb) + (size_t)(c0 + c) * d.rows + r0 + rr) = pack8(v);
    }
  }
}

}  // namespace

int launch_lora_project(const LoraMat* mats_dev, int m0, int m1, int strip_begin, int nstrips, int max_in, const float* grads_full, const float* lora,
                        float* lora_grads, float* scratch, int rank, float scale, hipStream_t s, const float* master, const float* norms) {
  if ((master == nullptr) != (norms == nullptr)) return fv_fail(FV_ERR_ARG, "lora_project: DoRA needs the master and the norms");
  if (!mats_dev || !grads_full || !lora || !lora_grads || !scratch || m1 <= m0 || nstrips <= 0 || rank < 1 || rank > 64 || max_in <= 0)
    return fv_fail(FV_ERR_ARG, "lora_project: bad arguments");
  for (int k0 = 0; k0 < rank; k0 += 32) {
    if (norms)
      hipLaunchKernelGGL(lora_project_kernel<1>, dim3((unsigned)nstrips), dim3(256), 0, s, mats_dev, m0, m1, strip_begin, grads_full, lora, lora_grads, scratch, rank,
                         k0, scale, master, norms);
    else
      hipLaunchKernelGGL(lora_project_kernel<0>, dim3((unsigned)nstrips), dim3(256), 0, s, mats_dev, m0, m1, strip_begin, grads_full, lora, lora_grads, scratch, rank,
                         k0, scale, nullptr, nullptr);
  }
  const unsigned gx = (unsigned)std::min<size_t>(((size_t)rank * max_in + 255) / 256, 1024);
  hipLaunchKernelGGL(lora_reduce_kernel, dim3(gx, (unsigned)(m1 - m0)), dim3(256), 0, s, mats_dev, m0, scratch, lora_grads, rank, scale);
  return hipGetLastError() == hipSuccess ? FV_OK : fv_fail(FV_ERR_HIP, "lora_project: launch failed");
}

int launch_lora_commit(const LoraCommitDesc* desc_dev, int ndesc, int ntiles, const LoraMat* mats_dev, const float* flat, const float* lora, int rank, float scale,
                       int f16_transposes, unsigned* sat, hipStream_t s, const float* norms) {
  if (!desc_dev || !mats_dev || !flat || !lora || ndesc <= 0 || ntiles <= 0 || rank < 1 || rank > 64 || !sat) return fv_fail(FV_ERR_ARG, "lora_commit: bad arguments");
  if (norms)
    hipLaunchKernelGGL((lora_commit_kernel<0, 1>), dim3((unsigned)ntiles), dim3(256), 0, s, desc_dev, ndesc, mats_dev, const_cast<float*>(flat), lora, rank, scale,
                       f16_transposes, sat, norms);
  else
    hipLaunchKernelGGL((lora_commit_kernel<0, 0>), dim3((unsigned)ntiles), dim3(256), 0, s, desc_dev, ndesc, mats_dev, const_cast<float*>(flat), lora, rank, scale,
                       f16_transposes, sat, nullptr);
  return hipGetLastError() == hipSuccess ? FV_OK : fv_fail(FV_ERR_HIP, "lora_commit: launch failed");
}

int launch_lora_merge(const LoraCommitDesc* desc_dev, int ndesc, int ntiles, const LoraMat* mats_dev, float* flat, const float* lora, int rank, float scale,
                      hipStream_t s, const float* norms) {
  if (!desc_dev || !mats_dev || !flat || !lora || ndesc <= 0 || ntiles <= 0 || rank < 1 || rank > 64) return fv_fail(FV_ERR_ARG, "lora_merge: bad arguments");
  if (norms)
    hipLaunchKernelGGL((lora_commit_kernel<1, 1>), dim3((unsigned)ntiles), dim3(256), 0, s, desc_dev, ndesc, mats_dev, flat, lora, rank, scale, 0, nullptr, norms);
  else
    hipLaunchKernelGGL((lora_commit_kernel<1, 0>), dim3((unsigned)ntiles), dim3(256), 0, s, desc_dev, ndesc, mats_dev, flat, lora, rank, scale, 0, nullptr, nullptr);
  return hipGetLastError() == hipSuccess ? FV_OK : fv_fail(FV_ERR_HIP, "lora_merge: launch failed");
}

int launch_lora_norms(const LoraCommitDesc* desc_dev, int ndesc, int nbands, const LoraMat* mats_dev, const float* flat, const float* lora, int rank, float scale,
                      float* norms, float* mag, hipStream_t s) {
  if (!desc_dev || !mats_dev || !flat || !lora || !norms || ndesc <= 0 || nbands <= 0 || rank < 1 || rank > 64) return fv_fail(FV_ERR_ARG, "lora_norms: bad arguments");
  hipLaunchKernelGGL(lora_norm_kernel, dim3((unsigned)nbands), dim3(256), 0, s, desc_dev, ndesc, mats_dev, flat, lora, rank, scale, norms, mag);
  return hipGetLastError() == hipSuccess ? FV_OK : fv_fail(FV_ERR_HIP, "lora_norms: launch failed");
}

}  // namespace fv
