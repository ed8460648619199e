// bnb.hip -- bitsandbytes 4-bit (NF4 / FP4, optional double-quantized absmax) matmul kernels, the blockwise dequantizer's launchers and the reference's
// bitsandbytes C ABI, MI355X / gfx950, wave64.
//
// Drop-in for mistralrs-quant/src/bitsandbytes/ffi.rs (the nine dequantize_blockwise_<T>_<type> symbols), behind BnbLinear (bitsandbytes/mod.rs), plus the
// stream-taking launchers launch_bnb_dequantize / launch_bnb_matmul that the native entry points of ext_bnb.hip forward to.  The format, the absmax rule and the
// element decode W_hat = RNE_T(f32(table[q] * A_b)) are in bnb_core.cuh.
//
// Output, every route: y[m][n] = RNE_T(sum_k f32(x[m][k]) f32(W_hat[n][k]) + f32(bias[n])), f32 accumulation, the bias added in f32 before the ONE rounding.
// W_hat is the rounded T value, so every route equals "dequantize, then matmul" on its operands.  Every output element is written once by a plain store; no
// atomics; the same launch gives the same bits.
//
// Routes (aligned: K % blocksize == 0 and a 16-byte aligned weight pointer, so a weight row is K / 2 contiguous 16-byte aligned bytes of whole blocks):
//   1  M <= 8, aligned            streaming GEMV: 32 lanes per weight row, 8 rows per workgroup; a lane streams 16 bytes (32 weights, one block) per step with
//                                 non-temporal loads, the next piece and its absmax in flight behind the current one's decode; the first piece is requested
//                                 before the workgroup stages anything.  The weight is read once for all M rows; activations are staged in LDS in chunks.  K is
//                                 split over gridDim.y workgroups where N alone does not fill the chip: the splits write f32 partials to a workspace and a
//                                 second kernel adds them in split order.  Split count and chunking depend on N and K only: a row of an M = 8 call has the
//                                 bits of its M = 1 call.
//   2  M > 8, aligned, bf16/f16   LDS-staged 64 x 128 x 128 tile on v_mfma_f32_32x32x16_{bf16,f16}: the packed B tile (128 rows x 64 bytes) is decoded once per
//                                 workgroup into LDS as T -- the W_hat values themselves; A = x; f32 accumulators; the bias in the epilogue.  The next packed
//                                 tile and its absmax are fetched into registers behind the MFMAs.
//   3  anything else              one wave per output element, flat-index nibble and absmax lookup.  Correct, untuned.
#include "bnb_core.cuh"

namespace mrs {

static int g_bnb_route = 0;

// ------------------------------------------------------------------------------------------------ route 1: streaming GEMV
constexpr int BNB_ROWS = 8;      // weight rows per 256-thread workgroup (32 lanes each)
constexpr int BNB_MAX_SPLIT = 8;
constexpr int BNB_TARGET_WGS = 2048;  // 8 workgroups per CU on 256 CUs
template <class T> constexpr int bnb_kc() { return sizeof(T) == 4 ? 1024 : 2048; }  // activation elements per row staged at a time (MR * 4 KiB of LDS)

template <class T> __device__ __forceinline__ int4 bnb_ld16_x(const T *p) {
  if constexpr (sizeof(T) == 4) return ld16_a4(p);
  else return ld16_a2(p);
}

// K splits: a function of N and K only.  A split holds at least 32 units (one 16-byte piece per lane of the row's 32).
static int bnb_splits(int N, int K) {
  const int wgs = (N + BNB_ROWS - 1) / BNB_ROWS, nu = K >> 5;
  int s = (BNB_TARGET_WGS + wgs - 1) / wgs;
  if (s > BNB_MAX_SPLIT) s = BNB_MAX_SPLIT;
  if (s > nu / 32) s = nu / 32;
  return s < 1 ? 1 : s;
}

template <class T, int MR>
__global__ void __launch_bounds__(256) bnb_gemv_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, BnbAbs ab, const T *__restrict__ bias,
                                                       T *__restrict__ y, float *__restrict__ ws, int M, int N, int K, int bshift, int qtype, int ups) {
  constexpr int KC = bnb_kc<T>(), UC = KC / 32, EPV = 16 / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) T xs[MR * KC];
  __shared__ float lut[BNB_LUT];
  const int tid = threadIdx.x, sub = tid & 31, row = blockIdx.x * BNB_ROWS + (tid >> 5);
  const bool live = row < N;
  const int n = live ? row : N - 1;  // lanes past N stream the last row again and write nothing
  const int nu = K >> 5, u0 = blockIdx.y * ups, u1 = min(nu, u0 + ups);
  const uint8_t *wr = w + (size_t)n * (size_t)(K >> 1);
  const long long e0 = (long long)n * K;
  // the stream starts before the workgroup stages anything
  int u = u0 + sub;
  int4 q = make_int4(0, 0, 0, 0);
  BnbAbsRaw ar = {0.0f, 0};
  if (u < u1) {
    q = ld16nt_a4(wr + (size_t)u * 16);
    ar = bnb_abs_fetch(ab, (e0 + 32LL * u) >> bshift);
  }
  bnb_fill_lut(lut, qtype, ab.nested_quant_map);
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.0f;
  for (int c0 = u0; c0 < u1; c0 += UC) {
    const int c1 = min(u1, c0 + UC), cv = (c1 - c0) * 32 / EPV;
    __syncthreads();  // the previous chunk's reads are done
    for (int i = tid; i < MR * cv; i += 256) {
      const int m = i / cv, c = i - m * cv;
      *(int4 *)(xs + m * KC + c * EPV) = m < M ? bnb_ld16_x<T>(x + (size_t)m * K + (size_t)c0 * 32 + c * EPV) : make_int4(0, 0, 0, 0);
    }
    __syncthreads();
    for (; u < c1; u += 32) {  // a lane's units are u0 + sub + 32 j and UC is a multiple of 32: the sequence carries over the chunks
      const int un = u + 32;
      int4 qn = make_int4(0, 0, 0, 0);
      BnbAbsRaw an = {0.0f, 0};
      if (un < u1) {
        qn = ld16nt_a4(wr + (size_t)un * 16);
        an = bnb_abs_fetch(ab, (e0 + 32LL * un) >> bshift);
      }
      const float A = bnb_abs_finish(ab, ar, lut);
      const uint32_t qq[4] = {(uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w};
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        float wf[8];
        bnb_word<T>(qq[jj], A, lut, wf);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          float a[8];
          afq_x8<T>(xs + m * KC + (u - c0) * 32 + jj * 8, a);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[m] = fmaf(a[e], wf[e], acc[m]);
        }
      }
      q = qn;
      ar = an;
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    float v = acc[m];
#pragma unroll
    for (int d = 16; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);  // stays inside the row's 32 lanes
    if (live && sub == 0 && m < M) {
      if (gridDim.y == 1) y[(size_t)m * N + n] = from_f<T>(v + (bias ? to_f<T>(bias[n]) : 0.0f));
      else ws[((size_t)blockIdx.y * M + m) * N + n] = v;
    }
  }
}

// second stage of a split launch: the partials of an output element are added in split order, then the bias, then the one rounding
template <class T>
__global__ void __launch_bounds__(256) bnb_split_sum_kernel(const float *__restrict__ ws, const T *__restrict__ bias, T *__restrict__ y, int MN, int N, int splits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= MN) return;
  float v = ws[i];
  for (int s = 1; s < splits; ++s) v += ws[(size_t)s * MN + i];
  y[i] = from_f<T>(v + (bias ? to_f<T>(bias[i % N]) : 0.0f));
}

template <class T, int MR>
static void bnb_gemv_rows(const T *x, const uint8_t *w, const BnbAbs &ab, const T *bias, T *y, float *ws, int M, int N, int K, int bshift, int qtype, int splits,
                          hipStream_t st) {
  const int nu = K >> 5, ups = (nu + splits - 1) / splits;
  hipLaunchKernelGGL((bnb_gemv_kernel<T, MR>), dim3((N + BNB_ROWS - 1) / BNB_ROWS, splits), dim3(256), 0, st, x, w, ab, bias, y, ws, M, N, K, bshift, qtype, ups);
  if (splits > 1) hipLaunchKernelGGL((bnb_split_sum_kernel<T>), dim3((M * N + 255) / 256), dim3(256), 0, st, (const float *)ws, bias, y, M * N, N, splits);
}

// ------------------------------------------------------------------------------------------------ route 2: MFMA tile on W_hat
constexpr int BTM = 64, BTN = 128, BTK = 128;
constexpr int BLD = BTK + 8;  // LDS row stride in 16-bit elements (272 B), as the AFQ tile: the 16-byte fragment reads of 32 consecutive rows spread over the banks
typedef __bf16 bnb_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 bnb_f16x8 __attribute__((ext_vector_type(8)));
typedef float bnb_f32x16 __attribute__((ext_vector_type(16)));

struct BnbTileLds {
  uint16_t a[BTM * BLD];  // x [row][k]
  uint16_t b[BTN * BLD];  // W_hat [n][k]
  float lut[BNB_LUT];
};

template <class T> __device__ __forceinline__ bnb_f32x16 bnb_mfma(const uint16_t *a, const uint16_t *b, bnb_f32x16 c) {
  if constexpr (__is_same(T, bf16_t))
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bnb_bf16x8 *)a, *(const bnb_bf16x8 *)b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const bnb_f16x8 *)a, *(const bnb_f16x8 *)b, c, 0, 0, 0);
}

// A operand = activations [row][k], B operand = W_hat [n][k]; lane l of a wave holds k = 8 (l >> 5) + j of row / column l & 31 in element j (as csrc/afq.hip).
template <class T>
__global__ void __launch_bounds__(256) bnb_tile_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, BnbAbs ab, const T *__restrict__ bias,
                                                       T *__restrict__ y, int M, int N, int K, int bshift, int qtype) {
  __shared__ __attribute__((aligned(16))) BnbTileLds L;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.y * BTM, n0 = blockIdx.x * BTN;
  // staging roles: A chunks (row (tid >> 4) + 16 i, 8 k at acol); B pieces (weight row (tid >> 2) + 64 i, the 16 bytes = 32 k at 32 (tid & 3))
  const int acol = (tid & 15) * 8, bk = (tid & 3) * 32;
  const T *arow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = m0 + (tid >> 4) + 16 * i;
    arow[i] = lr < M ? x + (size_t)lr * K : nullptr;
  }
  int brow[2];  // rows past N stage the last row again; their outputs are not written
#pragma unroll
  for (int i = 0; i < 2; ++i) brow[i] = min(n0 + (tid >> 2) + 64 * i, N - 1);

  int4 ra[4], rb[2];
  BnbAbsRaw rs[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = (arow[i] && k0 + acol < K) ? ld16_a2(arow[i] + k0 + acol) : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (k0 + bk < K) {  // K % 64 == 0: a piece is inside K or past it, never across
        const long long e = (long long)brow[i] * K + k0 + bk;
        rb[i] = ld16_a16(w + (e >> 1));
        rs[i] = bnb_abs_fetch(ab, e >> bshift);
      } else {
        rb[i] = make_int4(0, 0, 0, 0);
        rs[i] = BnbAbsRaw{0.0f, 0};
      }
    }
  };

  bnb_f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.0f;

  fetch(0);
  bnb_fill_lut(L.lut, qtype, ab.nested_quant_map);
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += BTK) {
    if (k0) __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) *(int4 *)&L.a[((tid >> 4) + 16 * i) * BLD + acol] = ra[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint16_t *dst = &L.b[((tid >> 2) + 64 * i) * BLD + bk];
      if (k0 + bk < K) {
        const float A = bnb_abs_finish(ab, rs[i], L.lut);
        const uint32_t qq[4] = {(uint32_t)rb[i].x, (uint32_t)rb[i].y, (uint32_t)rb[i].z, (uint32_t)rb[i].w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          float wf[8];
          bnb_word<T>(qq[jj], A, L.lut, wf);
          bnb_store8<T>((T *)(dst + 8 * jj), wf);
        }
      } else {  // past K: zeros against the zero-filled activations
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) *(int4 *)(dst + 8 * jj) = make_int4(0, 0, 0, 0);
      }
    }
    __syncthreads();
    if (k0 + BTK < K) fetch(k0 + BTK);  // in flight behind the MFMAs
    const int steps = (K - k0 < BTK ? K - k0 : BTK) >> 4;
    for (int s = 0; s < steps; ++s) {
      const int kk = 16 * s + 8 * h;
      const uint16_t *fb = &L.b[(wv * 32 + r) * BLD + kk];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) acc[mi] = bnb_mfma<T>(&L.a[(mi * 32 + r) * BLD + kk], fb, acc[mi]);
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
        if (lr < M) y[(size_t)lr * N + col] = from_f<T>(acc[mi][j] + bv);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ route 3: general
// One wave per output element; lane l takes k = l, l + 64, ...; element n K + k is nibble (n K + k) & 1 (0: high) of byte (n K + k) >> 1 in block
// (n K + k) / blocksize.  The lanes' f32 partials meet in a butterfly, so every lane holds the same sum.
template <class T>
__global__ void __launch_bounds__(256) bnb_general_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, BnbAbs ab, const T *__restrict__ bias,
                                                          T *__restrict__ y, int M, int N, int K, int bshift, int qtype) {
  __shared__ float lut[BNB_LUT];
  bnb_fill_lut(lut, qtype, ab.nested_quant_map);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= (long long)M * N) return;  // uniform over the wave
  const int m = (int)(o / N), n = (int)(o - (long long)m * N);
  const long long e0 = (long long)n * K;
  float acc = 0.0f;
  for (int k = lane; k < K; k += 64) {
    const long long e = e0 + k;
    const uint32_t b = w[e >> 1], qv = (e & 1) ? (b & 15u) : (b >> 4);
    const float A = bnb_abs_finish(ab, bnb_abs_fetch(ab, e >> bshift), lut);
    acc = fmaf(to_f<T>(x[(size_t)m * K + k]), round_to<T>(__fmul_rn(lut[qv], A)), acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) y[o] = from_f<T>(acc + (bias ? to_f<T>(bias[n]) : 0.0f));
}

// ------------------------------------------------------------------------------------------------ launchers
static bool bnb_abs_ok(const BnbAbs &ab) { return ab.absmax && (!ab.nested_absmax || (ab.nested_quant_map && ab.nested_blocksize > 0)); }

template <class T>
static int bnb_matmul(const void *x_, const void *w_, const BnbAbs &ab, const void *bias_, void *y_, float *ws, int M, int N, int K, int blocksize, int qtype,
                      void *stream) {
  const int bshift = bnb_block_shift(blocksize);
  if (!x_ || !w_ || !y_ || M < 0 || N < 0 || K <= 0 || bshift < 0 || (qtype != BNB_FP4 && qtype != BNB_NF4) || !bnb_abs_ok(ab)) return -1;
  if (M == 0 || N == 0) return 0;
  const T *x = (const T *)x_, *bias = (const T *)bias_;
  const uint8_t *w = (const uint8_t *)w_;
  T *y = (T *)y_;
  hipStream_t st = (hipStream_t)stream;
  const bool aligned = K % blocksize == 0 && ((uintptr_t)w & 15) == 0;
  if (M <= 8 && aligned) {
    int splits = bnb_splits(N, K);
    if (splits > 1 && !ws) return -1;  // the split is a function of N and K; a caller asks bnb_matmul_workspace_floats and brings the floats
    g_bnb_route = 1;
    // the register rows are padded to 1, 2, 4 or 8 (padding rows are staged as zeros and not written)
    if (M == 1) bnb_gemv_rows<T, 1>(x, w, ab, bias, y, ws, M, N, K, bshift, qtype, splits, st);
    else if (M == 2) bnb_gemv_rows<T, 2>(x, w, ab, bias, y, ws, M, N, K, bshift, qtype, splits, st);
    else if (M <= 4) bnb_gemv_rows<T, 4>(x, w, ab, bias, y, ws, M, N, K, bshift, qtype, splits, st);
    else bnb_gemv_rows<T, 8>(x, w, ab, bias, y, ws, M, N, K, bshift, qtype, splits, st);
  } else if (sizeof(T) == 2 && M > 8 && aligned) {
    if ((M + BTM - 1) / BTM > 65535) return -2;
    g_bnb_route = 2;
    if constexpr (sizeof(T) == 2)
      hipLaunchKernelGGL((bnb_tile_kernel<T>), dim3((N + BTN - 1) / BTN, (M + BTM - 1) / BTM), dim3(256), 0, st, x, w, ab, bias, y, M, N, K, bshift, qtype);
  } else {
    const long long grid = ((long long)M * N + 3) / 4;
    if (grid > 0x7fffffffLL) return -2;
    g_bnb_route = 3;
    hipLaunchKernelGGL((bnb_general_kernel<T>), dim3((unsigned)grid), dim3(256), 0, st, x, w, ab, bias, y, M, N, K, bshift, qtype);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mrs

extern "C" {

int launch_bnb_dequantize(const void *weight, const void *absmax, const float *code, const float *nested_absmax, const float *nested_quant_map, void *out,
                          long long n, int blocksize, int nested_blocksize, float nested_offset, int qtype, int dtype, void *stream) {
  const mrs::BnbAbs ab = {absmax, nested_absmax, nested_quant_map, nested_blocksize, nested_offset};
  if (dtype == 0) return mrs::bnb_dequant<float>(weight, ab, code, out, n, blocksize, qtype, (hipStream_t)stream);
  if (dtype == 1) return mrs::bnb_dequant<mrs::f16_t>(weight, ab, code, out, n, blocksize, qtype, (hipStream_t)stream);
  if (dtype == 2) return mrs::bnb_dequant<mrs::bf16_t>(weight, ab, code, out, n, blocksize, qtype, (hipStream_t)stream);
  return -1;
}

int launch_bnb_matmul(const void *x, const void *weight, const void *absmax, const float *nested_absmax, const float *nested_quant_map, const void *bias, void *y,
                      float *workspace, int M, int N, int K, int blocksize, int nested_blocksize, float nested_offset, int qtype, int dtype, void *stream) {
  const mrs::BnbAbs ab = {absmax, nested_absmax, nested_quant_map, nested_blocksize, nested_offset};
  if (dtype == 0) return mrs::bnb_matmul<float>(x, weight, ab, bias, y, workspace, M, N, K, blocksize, qtype, stream);
  if (dtype == 1) return mrs::bnb_matmul<mrs::f16_t>(x, weight, ab, bias, y, workspace, M, N, K, blocksize, qtype, stream);
  if (dtype == 2) return mrs::bnb_matmul<mrs::bf16_t>(x, weight, ab, bias, y, workspace, M, N, K, blocksize, qtype, stream);
  return -1;
}

long long bnb_matmul_workspace_floats(int M, int N, int K) {
  if (M <= 0 || M > 8 || N <= 0 || K <= 0) return 0;
  const int s = mrs::bnb_splits(N, K);
  return s > 1 ? (long long)s * M * N : 0;
}

int bnb_last_route(void) { return mrs::g_bnb_route; }

// ---- the reference's symbols (bitsandbytes/ffi.rs): plain f32 absmax, `n` output elements, no return value; `code` is read by the int8 type only
#define MRS_BNB_ABI(T, tag, name, QT)                                                                                                                   \
  void dequantize_blockwise_##tag##_##name(const float *code, const uint8_t *A, const float *absmax, T *out, int blocksize, int n, void *stream) {       \
    const mrs::BnbAbs ab = {absmax, nullptr, nullptr, 0, 0.0f};                                                                                         \
    (void)mrs::bnb_dequant_launch<T, QT>(A, ab, code, out, n, blocksize, (hipStream_t)stream);                                                          \
  }
#define MRS_BNB_ABI_T(T, tag) MRS_BNB_ABI(T, tag, int8, mrs::BNB_INT8) MRS_BNB_ABI(T, tag, fp4, mrs::BNB_FP4) MRS_BNB_ABI(T, tag, nf4, mrs::BNB_NF4)
MRS_BNB_ABI_T(float, f32)
MRS_BNB_ABI_T(mrs::f16_t, f16)
MRS_BNB_ABI_T(mrs::bf16_t, bf16)
#undef MRS_BNB_ABI_T
#undef MRS_BNB_ABI

}  // extern "C"
