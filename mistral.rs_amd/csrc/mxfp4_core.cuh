// mxfp4_core.cuh -- MXFP4 element decode shared by the matmul kernels (mxfp4.hip) and the dequantizer (ext_mxfp4.hip).
//
// Format (mistralrs-quant/src/mxfp4/mod.rs:19-36,589-609): a byte holds two E2M1 values, low nibble = element k, high nibble = k + 1;
// nibble magnitudes {0, .5, 1, 1.5, 2, 3, 4, 6}, bit 3 = sign; one E8M0 byte scales 32 consecutive k and means f32_from_bits(s << 23),
// so s = 0 is 0.0 (not 2^-127) exactly as the reference's DEQUANT_LUT.  value * scale is exact in f32 (2 significand bits times a power
// of two; f32 subnormals are kept), and its upper 16 bits are the same number as bf16 (the low 16 bits are zero).
#pragma once
#include "common.cuh"

namespace mrs {

__device__ __forceinline__ float mxfp4_scale(uint32_t s) { return __uint_as_float(s << 23); }

// nibble -> f32: the eight magnitudes as bf16 images in two 64-bit registers (entry m & 3 at bits 16 (m & 3)), no memory table
__device__ __forceinline__ float mxfp4_value(uint32_t nib) {
  constexpr uint64_t LO = 0x3FC03F803F000000ull;  // 1.5, 1, .5, 0
  constexpr uint64_t HI = 0x40C0408040404000ull;  // 6, 4, 3, 2
  const uint64_t t = (nib & 4u) ? HI : LO;
  const uint32_t mag = (uint32_t)(t >> ((nib & 3u) * 16u)) & 0xFFFFu;
  return __uint_as_float((mag << 16) | ((nib & 8u) << 28));
}

// one 32-bit word = 8 consecutive k -> 8 scaled f32 weights
__device__ __forceinline__ void mxfp4_word(uint32_t q, float s, float *w) {
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = mxfp4_value((q >> (4 * j)) & 15u) * s;
}

// two packed T (the low one first) -> f32
template <class T> __device__ __forceinline__ void unpack2(uint32_t v, float &a, float &b);
template <> __device__ __forceinline__ void unpack2<bf16_t>(uint32_t v, float &a, float &b) {
  a = __uint_as_float(v << 16);
  b = __uint_as_float(v & 0xFFFF0000u);
}
template <> __device__ __forceinline__ void unpack2<f16_t>(uint32_t v, float &a, float &b) {
  a = half_bits_to_float((uint16_t)(v & 0xFFFFu));
  b = half_bits_to_float((uint16_t)(v >> 16));
}

}  // namespace mrs
