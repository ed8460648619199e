// mxfp4.hip -- MXFP4 (E2M1 nibbles + E8M0 block scales, the GPT-OSS weight format) matmul and MoE gather kernels, MI355X / gfx950, wave64.
//
// Drop-in for the C ABI of mistralrs-quant/src/mxfp4/ffi.rs:7-31,59-127 (launch_mxfp4_matmul_{f16,bf16},
// launch_mxfp4_indexed_moe_gemm_{f16,bf16}, launch_mxfp4_moe_grouped_gemm_{f16,bf16}, mxfp4_get_max_smem_optin), behind MXFP4Layer::forward_raw /
// gather_forward_raw (mxfp4/mod.rs:106-182, ops.rs:16-214,313-614).  The *_wmma_* entry points are not provided: the reference gates them behind
// has_mxfp4_wmma_kernels, which a HIP build leaves unset.
//
// Numerics, every route: inputs -> f32, every product x * w exact in f32 (an 8- or 11-bit significand times a 2-bit one times a power of two),
// f32 accumulation, bias added in f32 after the K sum, one round-to-nearest-even conversion to the output type.  Expert ids >= num_experts read
// nothing and leave their output row untouched (kernels/mxfp4/mxfp4_gemm.cu:323-325).
//
// Routes:
//   1  dense, M <= 8          streaming GEMV: 32 lanes per weight row, one 16-byte block (32 k) per lane per step, the weight bytes are read once for
//                             all rows, activations staged per workgroup in 2048-k chunks.  The per-row order of the sum does not depend on M.
//   2  dense, M > 8, bf16     LDS-staged 64 x 128 x 64 tile on v_mfma_f32_32x32x16_bf16; weights are decoded once per workgroup into bf16 (the upper half
//                             of the f32 table[nibble] * scale, exact).
//   5  dense, M > 8, f16      route 1 over chunks of 8 rows (f16 weights cannot hold the scale range; the layer's dtype is bf16: correct, untuned).
//   3  MoE, <= 8 slots        route 1's kernel, one single-row GEMV per (token, slot), one launch.  Also taken when the slot list does not fit the LDS.
//   4  MoE, > 8 slots         grid (N tiles, experts): the workgroup gathers its expert's (token, slot) list from `indices` into LDS and runs route 2's
//                             tile body with indirect row reads and writes.  f16 activations are split x = hi + lo into two bf16 operands (8 + 3
//                             significand bits, both exact), so the products stay exact.
#include "mxfp4_core.cuh"

namespace mrs {

static int g_mxfp4_route = 0;

// ------------------------------------------------------------------------------------------------ route 1 / 3 / 5: streaming GEMV
constexpr int MX_KC = 2048;  // activation elements per row staged at a time
constexpr int MX_ROWS = 8;   // weight rows per 256-thread workgroup (32 lanes each)

template <class T, int MR, bool MOE>
__global__ void __launch_bounds__(256) mxfp4_gemv_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, const uint8_t *__restrict__ sc,
                                                         const T *__restrict__ bias, const uint32_t *__restrict__ indices, T *__restrict__ out, int N, int K,
                                                         int topk, int num_experts, int has_topk_dim, int slot0) {
  __shared__ __attribute__((aligned(16))) T xs[MR * MX_KC];
  const int nb = K >> 5;
  if constexpr (MOE) {
    const int slot = slot0 + blockIdx.y;
    const uint32_t e = indices[slot];
    if (e >= (uint32_t)num_experts) return;  // uniform over the workgroup
    x += (size_t)(has_topk_dim ? slot : slot / topk) * K;
    w += (size_t)e * N * (K >> 1);
    sc += (size_t)e * N * nb;
    if (bias) bias += (size_t)e * N;
    out += (size_t)slot * N;
  }
  const int tid = threadIdx.x, sub = tid & 31, n = blockIdx.x * MX_ROWS + (tid >> 5);
  const bool live = n < N;
  const uint8_t *wr = w + (size_t)(live ? n : 0) * (K >> 1);
  const uint8_t *sr = sc + (size_t)(live ? n : 0) * nb;  // a scale row starts at any byte: single-byte loads only
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += MX_KC) {
    const int kc = min(MX_KC, K - k0), c8 = kc >> 3;
    __syncthreads();
    for (int i = tid; i < MR * c8; i += 256) {
      const int m = i / c8, c = i - m * c8;
      *(int4 *)(xs + m * MX_KC + c * 8) = ld16_a2(x + (size_t)m * K + k0 + c * 8);
    }
    __syncthreads();
    if (live) {
      for (int b = sub; b < (kc >> 5); b += 32) {
        const int gb = (k0 >> 5) + b;
        const int4 q = ld16nt_a2(wr + (size_t)gb * 16);
        const float s = mxfp4_scale(sr[gb]);
        float wv[32];
        mxfp4_word((uint32_t)q.x, s, wv);
        mxfp4_word((uint32_t)q.y, s, wv + 8);
        mxfp4_word((uint32_t)q.z, s, wv + 16);
        mxfp4_word((uint32_t)q.w, s, wv + 24);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int4 xv = *(const int4 *)(xs + m * MX_KC + b * 32 + j * 8);
            float a0, a1;
            unpack2<T>((uint32_t)xv.x, a0, a1); acc[m] = fmaf(a0, wv[8 * j + 0], acc[m]); acc[m] = fmaf(a1, wv[8 * j + 1], acc[m]);
            unpack2<T>((uint32_t)xv.y, a0, a1); acc[m] = fmaf(a0, wv[8 * j + 2], acc[m]); acc[m] = fmaf(a1, wv[8 * j + 3], acc[m]);
            unpack2<T>((uint32_t)xv.z, a0, a1); acc[m] = fmaf(a0, wv[8 * j + 4], acc[m]); acc[m] = fmaf(a1, wv[8 * j + 5], acc[m]);
            unpack2<T>((uint32_t)xv.w, a0, a1); acc[m] = fmaf(a0, wv[8 * j + 6], acc[m]); acc[m] = fmaf(a1, wv[8 * j + 7], acc[m]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    float v = acc[m];
#pragma unroll
    for (int d = 16; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);  // stays inside the row's 32 lanes
    if (live && sub == 0) out[(size_t)m * N + n] = from_f<T>(v + (bias ? to_f<T>(bias[n]) : 0.0f));
  }
}

template <class T, int MR>
static void gemv_rows(const T *x, const uint8_t *w, const uint8_t *sc, const T *bias, T *out, int N, int K, hipStream_t st) {
  hipLaunchKernelGGL((mxfp4_gemv_kernel<T, MR, false>), dim3((N + MX_ROWS - 1) / MX_ROWS), dim3(256), 0, st, x, w, sc, bias, (const uint32_t *)nullptr, out,
                     N, K, 0, 0, 0, 0);
}

template <class T> static void gemv_dense(const T *x, const uint8_t *w, const uint8_t *sc, const T *bias, T *out, int M, int N, int K, hipStream_t st) {
  switch (M) {
  case 1: gemv_rows<T, 1>(x, w, sc, bias, out, N, K, st); break;
  case 2: gemv_rows<T, 2>(x, w, sc, bias, out, N, K, st); break;
  case 3: gemv_rows<T, 3>(x, w, sc, bias, out, N, K, st); break;
  case 4: gemv_rows<T, 4>(x, w, sc, bias, out, N, K, st); break;
  case 5: gemv_rows<T, 5>(x, w, sc, bias, out, N, K, st); break;
  case 6: gemv_rows<T, 6>(x, w, sc, bias, out, N, K, st); break;
  case 7: gemv_rows<T, 7>(x, w, sc, bias, out, N, K, st); break;
  default: gemv_rows<T, 8>(x, w, sc, bias, out, N, K, st); break;
  }
}

// ------------------------------------------------------------------------------------------------ route 2 / 4: bf16 MFMA tile
constexpr int TM = 64, TN = 128, TK = 64;
constexpr int TLD = TK + 8;  // LDS row stride in bf16 elements (144 B): the 16-byte fragment reads of 32 consecutive rows spread over the banks
typedef __bf16 mx_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mx_f32x16 __attribute__((ext_vector_type(16)));

template <class T> struct MxSplit { static constexpr int PARTS = 1; };
template <> struct MxSplit<f16_t> { static constexpr int PARTS = 2; };  // f16 = hi (upper 8 significand bits) + lo (the other 3), both exact bf16

// 8 T -> 8 bf16 (part 0) and, for f16, the 8 exact remainders (part 1)
template <class T> __device__ __forceinline__ void mx_a_parts(const int4 v, int4 &hi, int4 &lo) {
  if constexpr (MxSplit<T>::PARTS == 1) {
    hi = v;
    lo = make_int4(0, 0, 0, 0);
  } else {
    const uint32_t in[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
    uint32_t h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a, b;
      unpack2<f16_t>(in[i], a, b);
      const float ah = __uint_as_float(__float_as_uint(a) & 0xFFFF0000u), bh = __uint_as_float(__float_as_uint(b) & 0xFFFF0000u);
      h[i] = (__float_as_uint(ah) >> 16) | (__float_as_uint(bh) & 0xFFFF0000u);
      l[i] = (__float_as_uint(a - ah) >> 16) | (__float_as_uint(b - bh) & 0xFFFF0000u);  // <= 3 significand bits: the upper half is the value
    }
    hi = make_int4((int)h[0], (int)h[1], (int)h[2], (int)h[3]);
    lo = make_int4((int)l[0], (int)l[1], (int)l[2], (int)l[3]);
  }
}

// 8 nibbles -> 8 bf16 (upper halves of table * scale), packed
__device__ __forceinline__ int4 mx_b_word(uint32_t q, float s) {
  float w[8];
  mxfp4_word(q, s, w);
  uint32_t p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = (__float_as_uint(w[2 * i]) >> 16) | (__float_as_uint(w[2 * i + 1]) & 0xFFFF0000u);
  return make_int4((int)p[0], (int)p[1], (int)p[2], (int)p[3]);
}

template <int PARTS> struct MxTileLds {
  uint16_t a[PARTS][TM * TLD];
  uint16_t b[TN * TLD];
  int count;
};

// One TM x TN output tile.  Local row i of the tile is row rows[i] of the output (GATHER: a flat (token, slot) index from the expert's list) or m0 + i.
// A operand = activations [row][k], B operand = decoded weights [n][k]; lane l of a wave holds k = 8 (l >> 5) + j of row / column l & 31 in element j.
template <class T, bool GATHER>
__device__ __forceinline__ void mxfp4_tile(MxTileLds<MxSplit<T>::PARTS> &L, const int *list, const T *__restrict__ x, const uint8_t *__restrict__ w, const uint8_t *__restrict__ sc,
                                           const T *__restrict__ bias, T *__restrict__ out, int m0, int rows, int n0, int N, int K, int topk, int has_topk_dim) {
  constexpr int PARTS = MxSplit<T>::PARTS;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5, nb = K >> 5;
  // staging roles: A chunks (row, 8 k) tid and tid + 256; B block (weight row tid >> 1, k block tid & 1)
  const T *arow[2];
  int acol[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + 256 * i, lr = c >> 3;
    acol[i] = (c & 7) * 8;
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
  const int bn = n0 + (tid >> 1), bk = tid & 1;
  const bool blive = bn < N;
  const uint8_t *brow = w + (size_t)(blive ? bn : 0) * (K >> 1);
  const uint8_t *srow = sc + (size_t)(blive ? bn : 0) * nb;

  int4 ra[2], rb;
  float rs;
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) ra[i] = (arow[i] && k0 + acol[i] < K) ? ld16_a2(arow[i] + k0 + acol[i]) : make_int4(0, 0, 0, 0);
    const int gb = (k0 >> 5) + bk;
    const bool ok = blive && gb < nb;
    rb = ok ? ld16_a2(brow + (size_t)gb * 16) : make_int4(0, 0, 0, 0);
    rs = ok ? mxfp4_scale(srow[gb]) : 0.0f;
  };

  mx_f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.0f;

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += TK) {
    __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int4 hi, lo;
      mx_a_parts<T>(ra[i], hi, lo);
      const int off = ((tid + 256 * i) >> 3) * TLD + acol[i];
      *(int4 *)&L.a[0][off] = hi;
      if constexpr (PARTS == 2) *(int4 *)&L.a[1][off] = lo;
    }
    {
      uint16_t *dst = &L.b[(tid >> 1) * TLD + bk * 32];
      *(int4 *)(dst + 0) = mx_b_word((uint32_t)rb.x, rs);
      *(int4 *)(dst + 8) = mx_b_word((uint32_t)rb.y, rs);
      *(int4 *)(dst + 16) = mx_b_word((uint32_t)rb.z, rs);
      *(int4 *)(dst + 24) = mx_b_word((uint32_t)rb.w, rs);
    }
    __syncthreads();
    if (k0 + TK < K) fetch(k0 + TK);  // in flight behind the MFMAs
#pragma unroll
    for (int s = 0; s < TK / 16; ++s) {
      const int kk = 16 * s + 8 * h;
      const mx_bf16x8 fb = *(const mx_bf16x8 *)&L.b[(wv * 32 + r) * TLD + kk];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int p = 0; p < PARTS; ++p) {
          const mx_bf16x8 fa = *(const mx_bf16x8 *)&L.a[p][(mi * 32 + r) * TLD + kk];
          acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[mi], 0, 0, 0);
        }
      }
    }
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = n0 + wv * 32 + r;
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

template <class T>
__global__ void __launch_bounds__(256) mxfp4_tile_dense_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, const uint8_t *__restrict__ sc,
                                                               const T *__restrict__ bias, T *__restrict__ out, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) MxTileLds<MxSplit<T>::PARTS> L;
  mxfp4_tile<T, false>(L, nullptr, x, w, sc, bias, out, blockIdx.y * TM, M, blockIdx.x * TN, N, K, 1, 0);
}

template <class T>
__global__ void __launch_bounds__(256) mxfp4_tile_moe_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, const uint8_t *__restrict__ sc,
                                                             const T *__restrict__ bias, const uint32_t *__restrict__ indices, T *__restrict__ out, int total,
                                                             int topk, int N, int K, int has_topk_dim) {
  __shared__ __attribute__((aligned(16))) MxTileLds<MxSplit<T>::PARTS> L;
  extern __shared__ int mx_list[];  // [total]: the flat (token, slot) indices routed to this expert
  const int e = blockIdx.y, nb = K >> 5;
  if (threadIdx.x == 0) L.count = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += 256)
    if (indices[i] == (uint32_t)e) mx_list[atomicAdd(&L.count, 1)] = i;  // any order: a row's arithmetic does not depend on its place in the tile
  __syncthreads();
  const int rows = L.count;
  w += (size_t)e * N * (K >> 1);
  sc += (size_t)e * N * nb;
  if (bias) bias += (size_t)e * N;
  for (int m0 = 0; m0 < rows; m0 += TM) mxfp4_tile<T, true>(L, mx_list, x, w, sc, bias, out, m0, rows, blockIdx.x * TN, N, K, topk, has_topk_dim);
}

// ------------------------------------------------------------------------------------------------ launchers
static int max_lds() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess || v <= 0) {
    (void)hipGetLastError();
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return 0;
  }
  return v;
}

template <class T>
static void matmul(const void *input, const uint8_t *weight, const uint8_t *scale, const void *bias, void *output, int M, int N, int K, bool has_bias, void *stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (K & 31)) return;
  const T *x = (const T *)input, *b = has_bias ? (const T *)bias : nullptr;
  T *out = (T *)output;
  hipStream_t st = (hipStream_t)stream;
  if (M <= 8) {
    g_mxfp4_route = 1;
    gemv_dense<T>(x, weight, scale, b, out, M, N, K, st);
  } else if constexpr (MxSplit<T>::PARTS == 1) {
    g_mxfp4_route = 2;
    hipLaunchKernelGGL((mxfp4_tile_dense_kernel<T>), dim3((N + TN - 1) / TN, (M + TM - 1) / TM), dim3(256), 0, st, x, weight, scale, b, out, M, N, K);
  } else {
    g_mxfp4_route = 5;
    for (int r0 = 0; r0 < M; r0 += 8) gemv_dense<T>(x + (size_t)r0 * K, weight, scale, b, out + (size_t)r0 * N, min(8, M - r0), N, K, st);
  }
}

template <class T>
static void moe(const void *input, const uint8_t *weights, const uint8_t *scales, const void *biases, const uint32_t *indices, void *output, int num_tokens, int topk,
                int num_experts, int N, int K, bool has_bias, bool input_has_topk_dim, void *stream) {
  if (num_tokens <= 0 || topk <= 0 || num_experts <= 0 || N <= 0 || K <= 0 || (K & 31)) return;
  const T *x = (const T *)input, *b = has_bias ? (const T *)biases : nullptr;
  T *out = (T *)output;
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)num_tokens * topk;
  const long long list_bytes = total * 4, budget = (long long)max_lds() - (long long)sizeof(MxTileLds<MxSplit<T>::PARTS>) - 64;
  if (total > 8 && list_bytes <= budget && total <= 0x7fffffffLL) {
    g_mxfp4_route = 4;
    if (list_bytes > 32 * 1024) lds_attr_once((const void *)mxfp4_tile_moe_kernel<T>, (int)budget);
    hipLaunchKernelGGL((mxfp4_tile_moe_kernel<T>), dim3((N + TN - 1) / TN, num_experts), dim3(256), (size_t)list_bytes, st, x, weights, scales, b, indices, out,
                       (int)total, topk, N, K, (int)input_has_topk_dim);
    return;
  }
  g_mxfp4_route = 3;
  for (long long s0 = 0; s0 < total; s0 += 65535)  // grid.y limit
    hipLaunchKernelGGL((mxfp4_gemv_kernel<T, 1, true>), dim3((N + MX_ROWS - 1) / MX_ROWS, (unsigned)((total - s0) < 65535 ? (total - s0) : 65535)), dim3(256), 0, st, x,
                       weights, scales, b, indices, out, N, K, topk, num_experts, (int)input_has_topk_dim, (int)s0);
}

}  // namespace mrs

extern "C" {

void launch_mxfp4_matmul_f16(const void *input, const uint8_t *weight, const uint8_t *weight_scale, const void *bias, void *output, int M, int N, int K, bool has_bias,
                             void *stream) {
  mrs::matmul<mrs::f16_t>(input, weight, weight_scale, bias, output, M, N, K, has_bias, stream);
}
void launch_mxfp4_matmul_bf16(const void *input, const uint8_t *weight, const uint8_t *weight_scale, const void *bias, void *output, int M, int N, int K, bool has_bias,
                              void *stream) {
  mrs::matmul<mrs::bf16_t>(input, weight, weight_scale, bias, output, M, N, K, has_bias, stream);
}

#define MRS_MXFP4_MOE(name, T)                                                                                                                              \
  void name(const void *input, const uint8_t *weights, const uint8_t *weight_scales, const void *biases, const uint32_t *indices, void *output, int num_tokens, \
            int topk, int num_experts, int N, int K, bool has_bias, bool input_has_topk_dim, void *stream) {                                                  \
    mrs::moe<T>(input, weights, weight_scales, biases, indices, output, num_tokens, topk, num_experts, N, K, has_bias, input_has_topk_dim, stream);           \
  }
MRS_MXFP4_MOE(launch_mxfp4_indexed_moe_gemm_f16, mrs::f16_t)
MRS_MXFP4_MOE(launch_mxfp4_indexed_moe_gemm_bf16, mrs::bf16_t)
MRS_MXFP4_MOE(launch_mxfp4_moe_grouped_gemm_f16, mrs::f16_t)
MRS_MXFP4_MOE(launch_mxfp4_moe_grouped_gemm_bf16, mrs::bf16_t)
#undef MRS_MXFP4_MOE

int mxfp4_get_max_smem_optin(void) { return mrs::max_lds(); }
int mxfp4_last_route(void) { return mrs::g_mxfp4_route; }

}  // extern "C"
