// afq.hip -- AFQ (affine 2/3/4/6/8-bit) matmul and MoE gather kernels and the reference's AFQ C ABI, MI355X / gfx950, wave64.
//
// Drop-in for mistralrs-quant/src/afq/ffi.rs (afq_dequantize_*, afq_embedding_*, afq_quantize_*, afq_qmv_*, afq_qmm_*; no stream argument: the null
// stream), behind AfqLayer (afq/mod.rs) and afq/ops.rs, plus the stream-taking launchers launch_afq_matmul / launch_afq_indexed_moe_gemm that the native
// entry points of ext_afq.hip forward to.  The format and the dequantize / quantize rules are in afq_core.cuh.
//
// Numerics, every matmul route: inputs -> f32; per stretch of k inside one group, P = sum x q and X = sum x in f32 (q <= 255 is exact in bf16 / f16 / f32 and
// x q is exact in f32 for 16-bit x), then acc = fma(s, P, acc), acc = fma(b, X, acc) with the group's scale s and bias b; the optional output bias is added in
// f32 after the K sum; ONE round-to-nearest-even conversion to T.  The weight q s + b is never formed, so nothing rounds per element.  Expert ids >= num_experts
// read nothing and leave their output row untouched.
//
// Routes:
//   1  dense, M <= 8                    streaming GEMV: 32 lanes per weight row, one unit (32 k, `bits` words) per lane per step, stretch = the unit; the packed
//                                       words are read once for all rows (non-temporal, 4-byte alignment assumed), activations staged per workgroup in 2048-k
//                                       chunks.  The lane split and the chunking do not depend on M: a row of an M = 8 call has the bits of its M = 1 call.
//   2  dense, M > 8, bf16 / f16         LDS-staged 64 x 128 x 128 tile on v_mfma_f32_32x32x16_{bf16,f16}; the B operand is the code q, decoded once per
//                                       workgroup (one thread per unit); stretch = the group: P_g comes out of the matrix core, X_g from the staging threads'
//                                       unit sums.  Untuned: group 32 flushes every two MFMAs.
//   5  dense, M > 8, f32                route 1 over chunks of 8 rows (untuned).
//   3  MoE, <= 8 slots, or f32, or a slot list that does not fit the LDS: route 1's kernel, one single-row GEMV per (token, slot), one launch.
//   4  MoE otherwise                    grid (N tiles, experts): the workgroup gathers its expert's (token, slot) list from `indices` into dynamic LDS and
//                                       runs route 2's tile body with indirect row reads and writes.
#include "afq_core.cuh"

namespace mrs {

static int g_afq_route = 0;

// ------------------------------------------------------------------------------------------------ route 1 / 3 / 5: streaming GEMV
constexpr int AFQ_KC = 2048;  // activation elements per row staged at a time
constexpr int AFQ_ROWS = 8;   // weight rows per 256-thread workgroup (32 lanes each)

template <class T> __device__ __forceinline__ int4 afq_ld16_x(const T *p) {
  if constexpr (sizeof(T) == 4) return ld16_a4(p);
  else return ld16_a2(p);
}

template <class T, int BITS, int MR, bool MOE>
__global__ void __launch_bounds__(256) afq_gemv_kernel(const T *__restrict__ x, const uint32_t *__restrict__ w, const T *__restrict__ sc, const T *__restrict__ bi,
                                                       const T *__restrict__ bias, const uint32_t *__restrict__ indices, T *__restrict__ out, int M, int N, int K,
                                                       int gshift, int topk, int num_experts, int has_topk_dim, int slot0) {
  __shared__ __attribute__((aligned(16))) T xs[MR * AFQ_KC];
  constexpr int EPV = 16 / (int)sizeof(T);  // elements per 16-byte vector
  const int nu = K >> 5, ng = nu >> gshift;
  if constexpr (MOE) {
    const int slot = slot0 + blockIdx.y;
    const uint32_t e = indices[slot];
    if (e >= (uint32_t)num_experts) return;  // uniform over the workgroup
    x += (size_t)(has_topk_dim ? slot : slot / topk) * K;
    w += (size_t)e * N * nu * BITS;
    sc += (size_t)e * N * ng;
    bi += (size_t)e * N * ng;
    if (bias) bias += (size_t)e * N;
    out += (size_t)slot * N;
  }
  const int tid = threadIdx.x, sub = tid & 31, n = blockIdx.x * AFQ_ROWS + (tid >> 5);
  const bool live = n < N;
  const uint32_t *wr = w + (size_t)(live ? n : 0) * nu * BITS;
  const T *sr = sc + (size_t)(live ? n : 0) * ng, *br = bi + (size_t)(live ? n : 0) * ng;
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += AFQ_KC) {
    const int kc = min(AFQ_KC, K - k0), cv = kc / EPV;
    __syncthreads();
    for (int i = tid; i < MR * cv; i += 256) {
      const int m = i / cv, c = i - m * cv;
      *(int4 *)(xs + m * AFQ_KC + c * EPV) = m < M ? afq_ld16_x<T>(x + (size_t)m * K + k0 + c * EPV) : make_int4(0, 0, 0, 0);
    }
    __syncthreads();
    if (live) {
      for (int u = sub; u < (kc >> 5); u += 32) {
        const int gu = (k0 >> 5) + u;
        uint32_t wd[BITS];
        afq_load_unit<BITS, true>(wr + (size_t)gu * BITS, wd);
        const float s = to_f<T>(sr[gu >> gshift]), b = to_f<T>(br[gu >> gshift]);
        float P[MR], X[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) P[m] = X[m] = 0.0f;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          float q[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) q[e] = (float)afq_code<BITS>(wd, 8 * jj + e);
#pragma unroll
          for (int m = 0; m < MR; ++m) {
            float a[8];
            afq_x8<T>(xs + m * AFQ_KC + u * 32 + jj * 8, a);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              P[m] = fmaf(a[e], q[e], P[m]);
              X[m] += a[e];
            }
          }
        }
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          acc[m] = fmaf(s, P[m], acc[m]);
          acc[m] = fmaf(b, X[m], acc[m]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    float v = acc[m];
#pragma unroll
    for (int d = 16; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);  // stays inside the row's 32 lanes
    if (live && sub == 0 && m < M) out[(size_t)m * N + n] = from_f<T>(v + (bias ? to_f<T>(bias[n]) : 0.0f));
  }
}

template <class T, int BITS, int MR>
static void gemv_rows(const T *x, const uint32_t *w, const T *sc, const T *bi, const T *bias, T *out, int M, int N, int K, int gshift, hipStream_t st) {
  hipLaunchKernelGGL((afq_gemv_kernel<T, BITS, MR, false>), dim3((N + AFQ_ROWS - 1) / AFQ_ROWS), dim3(256), 0, st, x, w, sc, bi, bias, (const uint32_t *)nullptr,
                     out, M, N, K, gshift, 0, 0, 0, 0);
}

// M <= 8; the register rows are padded to 1, 2, 4 or 8 (padding rows are staged as zeros and not written)
template <class T, int BITS>
static void gemv_dense(const T *x, const uint32_t *w, const T *sc, const T *bi, const T *bias, T *out, int M, int N, int K, int gshift, hipStream_t st) {
  if (M == 1) gemv_rows<T, BITS, 1>(x, w, sc, bi, bias, out, M, N, K, gshift, st);
  else if (M == 2) gemv_rows<T, BITS, 2>(x, w, sc, bi, bias, out, M, N, K, gshift, st);
  else if (M <= 4) gemv_rows<T, BITS, 4>(x, w, sc, bi, bias, out, M, N, K, gshift, st);
  else gemv_rows<T, BITS, 8>(x, w, sc, bi, bias, out, M, N, K, gshift, st);
}

// ------------------------------------------------------------------------------------------------ route 2 / 4: MFMA tile on the codes
constexpr int ATM = 64, ATN = 128, ATK = 128;
constexpr int ALD = ATK + 8;  // LDS row stride in 16-bit elements (272 B): the 16-byte fragment reads of 32 consecutive rows spread over the banks
typedef __bf16 afq_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 afq_f16x8 __attribute__((ext_vector_type(8)));
typedef float afq_f32x16 __attribute__((ext_vector_type(16)));

struct AfqTileLds {
  uint16_t a[ATM * ALD];
  uint16_t b[ATN * ALD];
  float xu[ATM * 4];  // sum of x over each of the step's four units, per tile row
  int count;
};

template <class T> __device__ __forceinline__ uint32_t afq_code_bits(uint32_t q);  // the code as a T, exact
template <> __device__ __forceinline__ uint32_t afq_code_bits<bf16_t>(uint32_t q) { return __float_as_uint((float)q) >> 16; }
template <> __device__ __forceinline__ uint32_t afq_code_bits<f16_t>(uint32_t q) { return float_to_half_bits((float)q); }

template <class T> __device__ __forceinline__ afq_f32x16 afq_mfma(const uint16_t *a, const uint16_t *b, afq_f32x16 c) {
  if constexpr (__is_same(T, bf16_t))
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const afq_bf16x8 *)a, *(const afq_bf16x8 *)b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const afq_f16x8 *)a, *(const afq_f16x8 *)b, c, 0, 0, 0);
}

// One ATM x ATN output tile.  Local row i of the tile is row rows[i] of the output (GATHER: a flat (token, slot) index from the expert's list) or m0 + i.
// A operand = activations [row][k], B operand = codes [n][k]; lane l of a wave holds k = 8 (l >> 5) + j of row / column l & 31 in element j.
template <class T, int BITS, bool GATHER>
__device__ __forceinline__ void afq_tile(AfqTileLds &L, const int *list, const T *__restrict__ x, const uint32_t *__restrict__ w, const T *__restrict__ sc,
                                         const T *__restrict__ bi, const T *__restrict__ bias, T *__restrict__ out, int m0, int rows, int n0, int N, int K,
                                         int gshift, int topk, int has_topk_dim) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5, nu = K >> 5, ng = nu >> gshift;
  // staging roles: A chunks (row (tid >> 4) + 16 i, 8 k at acol); B units (weight row (tid >> 2) + 64 i, unit tid & 3)
  const int acol = (tid & 15) * 8, bu = tid & 3;
  const T *arow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = (tid >> 4) + 16 * i;
    arow[i] = nullptr;
    if (m0 + lr < rows) {
      int src = m0 + lr;
      if constexpr (GATHER) {
        const int slot = list[m0 + lr];
        src = has_topk_dim ? slot : slot / topk;
      }
      arow[i] = x + (size_t)src * K;
    }
  }
  const uint32_t *brow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int bn = n0 + (tid >> 2) + 64 * i;
    brow[i] = bn < N ? w + (size_t)bn * nu * BITS : nullptr;
  }

  int4 ra[4];
  uint32_t rb[2][BITS];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = (arow[i] && k0 + acol < K) ? ld16_a2(arow[i] + k0 + acol) : make_int4(0, 0, 0, 0);
    const int gu = (k0 >> 5) + bu;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (brow[i] && gu < nu) {
        afq_load_unit<BITS, false>(brow[i] + (size_t)gu * BITS, rb[i]);
      } else {
#pragma unroll
        for (int j = 0; j < BITS; ++j) rb[i][j] = 0u;
      }
    }
  };

  afq_f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.0f;
  const int col = n0 + wv * 32 + r;
  const T *scol = sc + (size_t)(col < N ? col : 0) * ng, *bcol = bi + (size_t)(col < N ? col : 0) * ng;
  const int glen = 32 << gshift;

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += ATK) {
    __syncthreads();  // the previous step's fragment and unit-sum reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = (tid >> 4) + 16 * i;
      *(int4 *)&L.a[lr * ALD + acol] = ra[i];
      float a0, a1, a2, a3, a4, a5, a6, a7;
      unpack2<T>((uint32_t)ra[i].x, a0, a1);
      unpack2<T>((uint32_t)ra[i].y, a2, a3);
      unpack2<T>((uint32_t)ra[i].z, a4, a5);
      unpack2<T>((uint32_t)ra[i].w, a6, a7);
      float s8 = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
      s8 += __shfl_xor(s8, 1, 64);
      s8 += __shfl_xor(s8, 2, 64);  // the four chunks of a unit sit in four adjacent lanes
      if ((tid & 3) == 0) L.xu[lr * 4 + ((tid & 15) >> 2)] = s8;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint16_t *dst = &L.b[((tid >> 2) + 64 * i) * ALD + bu * 32];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        uint32_t p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          p[e] = afq_code_bits<T>(afq_code<BITS>(rb[i], 8 * jj + 2 * e)) | (afq_code_bits<T>(afq_code<BITS>(rb[i], 8 * jj + 2 * e + 1)) << 16);
        *(int4 *)(dst + 8 * jj) = make_int4((int)p[0], (int)p[1], (int)p[2], (int)p[3]);
      }
    }
    __syncthreads();
    if (k0 + ATK < K) fetch(k0 + ATK);  // in flight behind the MFMAs
    for (int g = 0; g < (ATK >> 5 >> gshift); ++g) {
      const int gg = (k0 >> 5 >> gshift) + g;
      if (gg >= ng) break;  // uniform: the rest of the step lies past K and was staged as zeros
      afq_f32x16 P[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) P[i][j] = 0.0f;
      for (int s = 0; s < (glen >> 4); ++s) {
        const int kk = g * glen + 16 * s + 8 * h;
        const uint16_t *fb = &L.b[(wv * 32 + r) * ALD + kk];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) P[mi] = afq_mfma<T>(&L.a[(mi * 32 + r) * ALD + kk], fb, P[mi]);
      }
      const float sg = col < N ? to_f<T>(scol[gg]) : 0.0f, bg = col < N ? to_f<T>(bcol[gg]) : 0.0f;
      const int u0 = g << gshift, u1 = (g + 1) << gshift;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int lr = mi * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
          float X = L.xu[lr * 4 + u0];
          for (int u = u0 + 1; u < u1; ++u) X += L.xu[lr * 4 + u];
          acc[mi][j] = fmaf(sg, P[mi][j], acc[mi][j]);
          acc[mi][j] = fmaf(bg, X, acc[mi][j]);
        }
      }
    }
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  if (col < N) {
    const float bv = bias ? to_f<T>(bias[col]) : 0.0f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int lr = m0 + mi * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
        if (lr < rows) {
          int dst = lr;
          if constexpr (GATHER) dst = list[lr];
          out[(size_t)dst * N + col] = from_f<T>(acc[mi][j] + bv);
        }
      }
    }
  }
}

template <class T, int BITS>
__global__ void __launch_bounds__(256) afq_tile_dense_kernel(const T *__restrict__ x, const uint32_t *__restrict__ w, const T *__restrict__ sc, const T *__restrict__ bi,
                                                             const T *__restrict__ bias, T *__restrict__ out, int M, int N, int K, int gshift) {
  __shared__ __attribute__((aligned(16))) AfqTileLds L;
  afq_tile<T, BITS, false>(L, nullptr, x, w, sc, bi, bias, out, blockIdx.y * ATM, M, blockIdx.x * ATN, N, K, gshift, 1, 0);
}

template <class T, int BITS>
__global__ void __launch_bounds__(256) afq_tile_moe_kernel(const T *__restrict__ x, const uint32_t *__restrict__ w, const T *__restrict__ sc, const T *__restrict__ bi,
                                                           const T *__restrict__ bias, const uint32_t *__restrict__ indices, T *__restrict__ out, int total, int topk,
                                                           int N, int K, int gshift, int has_topk_dim) {
  __shared__ __attribute__((aligned(16))) AfqTileLds L;
  extern __shared__ int afq_list[];  // [total]: the flat (token, slot) indices routed to this expert
  const int e = blockIdx.y, nu = K >> 5, ng = nu >> gshift;
  if (threadIdx.x == 0) L.count = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += 256)
    if (indices[i] == (uint32_t)e) afq_list[atomicAdd(&L.count, 1)] = i;  // any order: a row's arithmetic does not depend on its place in the tile
  __syncthreads();
  const int rows = L.count;
  w += (size_t)e * N * nu * BITS;
  sc += (size_t)e * N * ng;
  bi += (size_t)e * N * ng;
  if (bias) bias += (size_t)e * N;
  for (int m0 = 0; m0 < rows; m0 += ATM) afq_tile<T, BITS, true>(L, afq_list, x, w, sc, bi, bias, out, m0, rows, blockIdx.x * ATN, N, K, gshift, topk, has_topk_dim);
}

// ------------------------------------------------------------------------------------------------ launchers
static int afq_max_lds() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess || v <= 0) {
    (void)hipGetLastError();
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return 0;
  }
  return v;
}

template <class T, int BITS>
static void matmul_bits(const T *x, const uint32_t *w, const T *sc, const T *bi, const T *bias, T *out, int M, int N, int K, int gshift, hipStream_t st) {
  if (M <= 8) {
    g_afq_route = 1;
    gemv_dense<T, BITS>(x, w, sc, bi, bias, out, M, N, K, gshift, st);
  } else if constexpr (sizeof(T) == 2) {
    g_afq_route = 2;
    hipLaunchKernelGGL((afq_tile_dense_kernel<T, BITS>), dim3((N + ATN - 1) / ATN, (M + ATM - 1) / ATM), dim3(256), 0, st, x, w, sc, bi, bias, out, M, N, K, gshift);
  } else {
    g_afq_route = 5;
    for (int r0 = 0; r0 < M; r0 += 8) gemv_dense<T, BITS>(x + (size_t)r0 * K, w, sc, bi, bias, out + (size_t)r0 * N, min(8, M - r0), N, K, gshift, st);
  }
}

template <class T, int BITS>
static void moe_bits(const T *x, const uint32_t *w, const T *sc, const T *bi, const T *bias, const uint32_t *indices, T *out, int num_tokens, int topk, int num_experts,
                     int N, int K, int gshift, int has_topk_dim, hipStream_t st) {
  const long long total = (long long)num_tokens * topk;
  if constexpr (sizeof(T) == 2) {
    const long long list_bytes = total * 4, budget = (long long)afq_max_lds() - (long long)sizeof(AfqTileLds) - 64;
    if (total > 8 && list_bytes <= budget && total <= 0x7fffffffLL) {
      g_afq_route = 4;
      if (list_bytes > 8 * 1024) lds_attr_once((const void *)afq_tile_moe_kernel<T, BITS>, (int)budget);
      hipLaunchKernelGGL((afq_tile_moe_kernel<T, BITS>), dim3((N + ATN - 1) / ATN, num_experts), dim3(256), (size_t)list_bytes, st, x, w, sc, bi, bias, indices, out,
                         (int)total, topk, N, K, gshift, has_topk_dim);
      return;
    }
  }
  g_afq_route = 3;
  for (long long s0 = 0; s0 < total; s0 += 65535)  // grid.y limit
    hipLaunchKernelGGL((afq_gemv_kernel<T, BITS, 1, true>), dim3((N + AFQ_ROWS - 1) / AFQ_ROWS, (unsigned)((total - s0) < 65535 ? (total - s0) : 65535)), dim3(256), 0,
                       st, x, w, sc, bi, bias, indices, out, 1, N, K, gshift, topk, num_experts, has_topk_dim, (int)s0);
}

template <class T>
static int matmul(const void *x, const void *w, const void *sc, const void *bi, const void *bias, void *out, int M, int N, int K, int bits, int group, void *stream) {
  const int gs = afq_group_shift(group);
  if (!x || !w || !sc || !bi || !out || M < 0 || N < 0 || K <= 0 || !afq_bits_ok(bits) || gs < 0 || K % group) return -1;
  if (M == 0 || N == 0) return 0;
#define MRS_AFQ_MM(B) matmul_bits<T, B>((const T *)x, (const uint32_t *)w, (const T *)sc, (const T *)bi, (const T *)bias, (T *)out, M, N, K, gs, (hipStream_t)stream)
  switch (bits) {
  case 2: MRS_AFQ_MM(2); break;
  case 3: MRS_AFQ_MM(3); break;
  case 4: MRS_AFQ_MM(4); break;
  case 6: MRS_AFQ_MM(6); break;
  default: MRS_AFQ_MM(8); break;
  }
#undef MRS_AFQ_MM
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <class T>
static int moe(const void *x, const void *w, const void *sc, const void *bi, const void *bias, const uint32_t *indices, void *out, int num_tokens, int topk,
               int num_experts, int N, int K, int bits, int group, int has_topk_dim, void *stream) {
  const int gs = afq_group_shift(group);
  if (!x || !w || !sc || !bi || !indices || !out || num_tokens < 0 || topk < 0 || num_experts <= 0 || N < 0 || K <= 0 || !afq_bits_ok(bits) || gs < 0 || K % group)
    return -1;
  if (num_tokens == 0 || topk == 0 || N == 0) return 0;
#define MRS_AFQ_MOE(B)                                                                                                                                       \
  moe_bits<T, B>((const T *)x, (const uint32_t *)w, (const T *)sc, (const T *)bi, (const T *)bias, indices, (T *)out, num_tokens, topk, num_experts, N, K, gs, \
                 has_topk_dim, (hipStream_t)stream)
  switch (bits) {
  case 2: MRS_AFQ_MOE(2); break;
  case 3: MRS_AFQ_MOE(3); break;
  case 4: MRS_AFQ_MOE(4); break;
  case 6: MRS_AFQ_MOE(6); break;
  default: MRS_AFQ_MOE(8); break;
  }
#undef MRS_AFQ_MOE
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mrs

extern "C" {

int launch_afq_matmul(const void *x, const void *w_q, const void *scales, const void *biases, const void *bias, void *y, int M, int N, int K, int bits, int group,
                      int dtype, void *stream) {
  if (dtype == 0) return mrs::matmul<float>(x, w_q, scales, biases, bias, y, M, N, K, bits, group, stream);
  if (dtype == 1) return mrs::matmul<mrs::f16_t>(x, w_q, scales, biases, bias, y, M, N, K, bits, group, stream);
  if (dtype == 2) return mrs::matmul<mrs::bf16_t>(x, w_q, scales, biases, bias, y, M, N, K, bits, group, stream);
  return -1;
}

int launch_afq_indexed_moe_gemm(const void *x, const void *w_q, const void *scales, const void *biases, const void *bias, const uint32_t *indices, void *y,
                                int num_tokens, int topk, int num_experts, int N, int K, int bits, int group, int dtype, int input_has_topk_dim, void *stream) {
  if (dtype == 0) return mrs::moe<float>(x, w_q, scales, biases, bias, indices, y, num_tokens, topk, num_experts, N, K, bits, group, input_has_topk_dim, stream);
  if (dtype == 1) return mrs::moe<mrs::f16_t>(x, w_q, scales, biases, bias, indices, y, num_tokens, topk, num_experts, N, K, bits, group, input_has_topk_dim, stream);
  if (dtype == 2) return mrs::moe<mrs::bf16_t>(x, w_q, scales, biases, bias, indices, y, num_tokens, topk, num_experts, N, K, bits, group, input_has_topk_dim, stream);
  return -1;
}

int afq_last_route(void) { return mrs::g_afq_route; }

// ---- the reference's symbols (afq/ffi.rs): null stream, no return value
#define MRS_AFQ_ABI(B, G, T, tag, WQ)                                                                                                                  \
  void afq_dequantize_##B##bit_gs##G##_##tag(const WQ *w_q, const T *scales, const T *biases, T *output, int rows, int cols) {                         \
    (void)mrs::afq_dequant_rows<T>(w_q, scales, biases, nullptr, output, rows, cols, B, G, nullptr);                                                   \
  }                                                                                                                                                    \
  void afq_embedding_##B##bit_gs##G##_##tag(const uint8_t *w_q, const T *scales, const T *biases, const uint32_t *ids, T *output, int num_ids, int hidden) { \
    (void)mrs::afq_dequant_rows<T>(w_q, scales, biases, ids, output, num_ids, hidden, B, G, nullptr);                                                  \
  }                                                                                                                                                    \
  void afq_qmv_##B##bit_gs##G##_##tag(const T *x, const WQ *w_q, const T *scales, const T *biases, T *y, int m, int n, int k) {                         \
    (void)mrs::matmul<T>(x, w_q, scales, biases, nullptr, y, m, n, k, B, G, nullptr);                                                                  \
  }
#define MRS_AFQ_ABI_P2(B, G, T, tag)                                                                                                                   \
  MRS_AFQ_ABI(B, G, T, tag, uint32_t)                                                                                                                  \
  void afq_quantize_##B##bit_gs##G##_##tag(const T *w, uint32_t *w_q, T *scales, T *biases, int rows, int cols) {                                      \
    (void)mrs::afq_quantize<T>(w, w_q, scales, biases, rows, cols, B, G, nullptr);                                                                     \
  }                                                                                                                                                    \
  void afq_qmm_##B##bit_gs##G##_##tag(const T *x, const uint32_t *w_q, const T *scales, const T *biases, T *y, int m, int n, int k) {                   \
    (void)mrs::matmul<T>(x, w_q, scales, biases, nullptr, y, m, n, k, B, G, nullptr);                                                                  \
  }
#define MRS_AFQ_ABI_G(G, T, tag)                                                                                                                       \
  MRS_AFQ_ABI_P2(2, G, T, tag) MRS_AFQ_ABI(3, G, T, tag, uint8_t) MRS_AFQ_ABI_P2(4, G, T, tag) MRS_AFQ_ABI(6, G, T, tag, uint8_t) MRS_AFQ_ABI_P2(8, G, T, tag)
#define MRS_AFQ_ABI_T(T, tag) MRS_AFQ_ABI_G(32, T, tag) MRS_AFQ_ABI_G(64, T, tag) MRS_AFQ_ABI_G(128, T, tag)
MRS_AFQ_ABI_T(float, f32)
MRS_AFQ_ABI_T(mrs::f16_t, f16)
MRS_AFQ_ABI_T(mrs::bf16_t, bf16)
#undef MRS_AFQ_ABI_T
#undef MRS_AFQ_ABI_G
#undef MRS_AFQ_ABI_P2
#undef MRS_AFQ_ABI

}  // extern "C"
