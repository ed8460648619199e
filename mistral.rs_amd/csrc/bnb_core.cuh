// bnb_core.cuh -- bitsandbytes blockwise formats (NF4, FP4, 8-bit dynamic map): tables, absmax of a block, element decode and the dequantize kernel, shared by
// the matmul kernels of bnb.hip.
//
// Format: 4-bit `weight` is the flat row-major [N, K] tensor, two elements per byte, element 2 i in the HIGH nibble of byte i and element 2 i + 1 in
// the low one; (n + 1) / 2 bytes for n elements.  Block b covers flat elements [b * blocksize, (b + 1) * blocksize) whatever the row length (a block may straddle
// rows); blocksize is a power of two in [64, 4096].  The 8-bit type is one code per byte and a caller-supplied 256-entry f32 map.
//
// absmax of block b: plain f32 absmax[b], or (double quantization) absmax is u8 and
//     A_b = f32(f32(nested_quant_map[absmax[b]] * nested_absmax[b / nested_blocksize]) + nested_offset)
// one f32 multiply and one f32 add, never contracted.  Decode: W_hat = RNE_T(f32(table[q] * A_b)).  The FP4 table carries the sign in the entry (entry 8 is
// -0.0): IEEE multiplication gives sign(a) xor sign(b) and the magnitude of |a| |b|, so this has the bits of "sign applied after the product".
#pragma once
#include "afq_core.cuh"  // afq_x8, unpack2

namespace mrs {

enum { BNB_INT8 = 0, BNB_FP4 = 1, BNB_NF4 = 2 };  // the reference's DataType_t

// The published 4-bit code books.  NF4: the 16 NormalFloat4 levels (QLoRA, appendix E) as f32.  FP4: sign | index into {0, 2^-6 / 3, 2/3, 1, 1/3, 1/2, 1/6, 1/4}
// as the f32 literals the format publishes (0.0052083333, 0.66666667, ...).
__device__ static const float BNB_TABLE[2][16] = {
    // FP4
    {0.0f, 5.208333333e-03f, 0.66666667f, 1.0f, 0.33333333f, 0.5f, 0.16666667f, 0.25f,  //
     -0.0f, -5.208333333e-03f, -0.66666667f, -1.0f, -0.33333333f, -0.5f, -0.16666667f, -0.25f},
    // NF4
    {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
     0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f,
     1.0f}};

__host__ __device__ constexpr int bnb_block_shift(int bs) {
  return bs == 64 ? 6 : bs == 128 ? 7 : bs == 256 ? 8 : bs == 512 ? 9 : bs == 1024 ? 10 : bs == 2048 ? 11 : bs == 4096 ? 12 : -1;
}

// Where a block's absmax comes from.  nested_absmax == nullptr: `absmax` is f32.  Otherwise `absmax` is u8 and the three nested fields are used.
struct BnbAbs {
  const void *absmax;
  const float *nested_absmax;
  const float *nested_quant_map;  // 256 f32
  int nested_blocksize;
  float nested_offset;
};

constexpr int BNB_LUT = 16 + 256;  // LDS floats: the 16-entry code book, then the 256-entry map (nested_quant_map, or the 8-bit type's code)

// Fills the workgroup's tables (256 threads); the caller synchronises before the first lookup.  A 16-dword LDS table is conflict-free by construction: lanes that
// read the same entry are served by a broadcast and different entries lie in different banks.
__device__ __forceinline__ void bnb_fill_lut(float *lut, int qtype, const float *map256) {
  const int tid = threadIdx.x;
  if (tid < 16) lut[tid] = BNB_TABLE[qtype == BNB_NF4 ? 1 : 0][tid];
  if (map256 && tid < 256) lut[16 + tid] = map256[tid];
}

// The global half of an absmax lookup (issued early, next to the weight load), and the LDS half that turns it into A_b.
struct BnbAbsRaw {
  float a;  // plain: absmax[b]; nested: nested_absmax[b / nested_blocksize]
  int c;    // nested: the u8 code absmax[b]
};
__device__ __forceinline__ BnbAbsRaw bnb_abs_fetch(const BnbAbs &ab, long long b) {
  BnbAbsRaw r;
  if (ab.nested_absmax) {
    r.c = ((const uint8_t *)ab.absmax)[b];
    r.a = ab.nested_absmax[b / ab.nested_blocksize];
  } else {
    r.c = 0;
    r.a = ((const float *)ab.absmax)[b];
  }
  return r;
}
__device__ __forceinline__ float bnb_abs_finish(const BnbAbs &ab, const BnbAbsRaw &r, const float *lut) {
  return ab.nested_absmax ? __fadd_rn(__fmul_rn(lut[16 + r.c], r.a), ab.nested_offset) : r.a;
}

// 8 consecutive elements (4 bytes, one little-endian word) -> the f32 values of W_hat
template <class T> __device__ __forceinline__ void bnb_word(uint32_t q, float A, const float *lut, float (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t b = (q >> (8 * j)) & 0xffu;
    w[2 * j] = round_to<T>(__fmul_rn(lut[b >> 4], A));
    w[2 * j + 1] = round_to<T>(__fmul_rn(lut[b & 15u], A));
  }
}

// 8 f32 values that are already T values -> 8 T at a 16-byte aligned address (two 16-byte pieces for f32)
template <class T> __device__ __forceinline__ void bnb_store8(T *dst, const float (&w)[8]) {
  if constexpr (sizeof(T) == 4) {
    *(float4 *)dst = make_float4(w[0], w[1], w[2], w[3]);
    *(float4 *)(dst + 4) = make_float4(w[4], w[5], w[6], w[7]);
  } else {
    uint32_t p[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const T lo = from_f<T>(w[2 * e]), hi = from_f<T>(w[2 * e + 1]);
      p[e] = (uint32_t)__builtin_bit_cast(uint16_t, lo) | ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
    }
    *(int4 *)dst = make_int4((int)p[0], (int)p[1], (int)p[2], (int)p[3]);
  }
}

// ------------------------------------------------------------------------------------------------ dequantize
// A thread owns 16 bytes of `weight`: 32 elements (4-bit) or 16 (8-bit), always inside one block, written as whole 16-byte pieces.  The thread that holds the
// end of the tensor (a partial piece, or the odd last element), and every thread when `vec` is 0 (a pointer that is not 16-byte aligned), goes element by element
// and writes nothing past n.  The nested absmax is computed here: the double-quantized dequantize is this one launch.
template <class T, int QT>
__global__ void __launch_bounds__(256) bnb_dequant_kernel(const uint8_t *__restrict__ w, BnbAbs ab, const float *__restrict__ code, T *__restrict__ out, long long n,
                                                          int bshift, int vec) {
  __shared__ float lut[BNB_LUT];
  constexpr int EPT = QT == BNB_INT8 ? 16 : 32;  // elements per thread
  bnb_fill_lut(lut, QT, QT == BNB_INT8 ? code : ab.nested_quant_map);
  __syncthreads();
  const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * EPT;
  if (e0 >= n) return;
  const float A = bnb_abs_finish(ab, bnb_abs_fetch(ab, e0 >> bshift), lut);
  const uint8_t *src = w + (QT == BNB_INT8 ? e0 : e0 >> 1);
  T *dst = out + e0;
  if (vec && e0 + EPT <= n) {
    const int4 v = ld16_a16(src);
    const uint32_t q[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
    if constexpr (QT == BNB_INT8) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = round_to<T>(__fmul_rn(lut[16 + ((q[2 * h + (e >> 2)] >> (8 * (e & 3))) & 0xffu)], A));
        bnb_store8<T>(dst + 8 * h, f);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float f[8];
        bnb_word<T>(q[j], A, lut, f);
        bnb_store8<T>(dst + 8 * j, f);
      }
    }
    return;
  }
  const int cnt = (int)(n - e0 < EPT ? n - e0 : EPT);
  for (int e = 0; e < cnt; ++e) {
    float t;
    if constexpr (QT == BNB_INT8) t = lut[16 + src[e]];
    else t = lut[(e & 1) ? (src[e >> 1] & 15u) : (src[e >> 1] >> 4)];
    dst[e] = from_f<T>(__fmul_rn(t, A));
  }
}

template <class T, int QT> static int bnb_dequant_launch(const void *w, const BnbAbs &ab, const float *code, void *out, long long n, int blocksize, hipStream_t st) {
  const int bshift = bnb_block_shift(blocksize);
  if (!w || !ab.absmax || !out || n < 0 || bshift < 0 || (QT == BNB_INT8 && (!code || ab.nested_absmax)) ||
      (ab.nested_absmax && (!ab.nested_quant_map || ab.nested_blocksize <= 0)))
    return -1;
  if (n == 0) return 0;
  constexpr int EPT = QT == BNB_INT8 ? 16 : 32;
  const long long grid = ((n + EPT - 1) / EPT + 255) / 256;
  if (grid > 0x7fffffffLL) return -2;
  const int vec = (((uintptr_t)w | (uintptr_t)out) & 15) == 0;
  hipLaunchKernelGGL((bnb_dequant_kernel<T, QT>), dim3((unsigned)grid), dim3(256), 0, st, (const uint8_t *)w, ab, code, (T *)out, n, bshift, vec);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <class T> static int bnb_dequant(const void *w, const BnbAbs &ab, const float *code, void *out, long long n, int blocksize, int qtype, hipStream_t st) {
  if (qtype == BNB_INT8) return bnb_dequant_launch<T, BNB_INT8>(w, ab, code, out, n, blocksize, st);
  if (qtype == BNB_FP4) return bnb_dequant_launch<T, BNB_FP4>(w, ab, code, out, n, blocksize, st);
  if (qtype == BNB_NF4) return bnb_dequant_launch<T, BNB_NF4>(w, ab, code, out, n, blocksize, st);
  return -1;
}

}  // namespace mrs
