// blockwise_fp8.hip -- blockwise FP8 (OCP E4M3 bytes + one f32 scale per weight block, the DeepSeek-V3 / Qwen3-FP8 checkpoint format) dequantize, quantize,
// matmul and MoE gather kernels, MI355X / gfx950, wave64.
//
// Drop-in for the C ABI of mistralrs-quant/src/blockwise_fp8/ffi.rs:127-271 (launch_dequant_fp8_blockwise_kernel_{f32,f16,bf16},
// launch_quant_fp8_blockwise_kernel_{f32,f16,bf16}, launch_fp8_matmul_{f16,bf16}, launch_fp8_indexed_moe_gemm_{f16,bf16}), behind
// BlockwiseFP8Linear::forward / gather_forward / dequantize_w (blockwise_fp8/mod.rs:180-317, ops.rs).  The sm90 entry points (mistralrs_cutlass_fp8_*,
// mistralrs_deepgemm_*, mistralrs_fp8_quantize_activation_*) are not provided: the reference gates them behind cfgs that a HIP build leaves unset.
//
// Format: weight [N][K] bytes, OCP E4M3FN (bias 7, no infinities, 0x7f / 0xff NaN, max 448); scale f32 [ceil(N / bsy)][scale_row_stride], element (n, k) uses
// scale[(n / bsy) * stride + k / bsx]; experts: weight [E][N][K], the scale of expert e starts at e * ceil(N / bsy) * stride.  Block sizes are any positive
// integers; N, K need not be multiples of them.
//
// Numerics.  Dequantize: T(f32(w) * scale), one f32 product and one conversion.  Quantize (kernels/blockwise_fp8/blockwise_fp8.cu:68-139): scale =
// max(absmax / 448, 1e-12) with the correctly rounded f32 division, q = e4m3_satfinite_rne(f16_rne(clamp(f32(v) / scale, +-448))); the double rounding is the
// reference's.  Matmul / MoE: inputs -> f32, every product x * w exact (an 8- or 11-bit significand times a 4-bit one); the products of one scale block (on
// the GEMV: of each 16-k piece of one) are summed in f32, that partial sum goes into the running f32 sum as fma(scale, partial, total), one
// round-to-nearest-even conversion to T at the end.  The scale stays outside the 16-bit MFMA, so its operands are the unscaled E4M3 values, exact in bf16 and
// in f16.  No bias in the ABI.  Expert ids >= num_experts read nothing and leave their output row untouched (blockwise_fp8_gemm.cu:153-155).  The matmul
// routes decode with v_cvt_pk_f32_fp8 (OCP on gfx950; a NaN byte stays a NaN); dequantize uses the integer definition of common.cuh.
//
// Routes (fp8_blockwise_last_route).  "fast" means: K % 16 == 0, block_size_x % 16 == 0 (a 16-byte load and an MFMA k step never straddle two scale
// blocks) and a 16-byte aligned weight base.  Activations may be aligned to their element only.
//   1  dense, fast, M <= 8     streaming GEMV: 32 lanes per weight row, one 16-byte non-temporal load (16 k) per lane per step, the weight bytes are read once
//                              for all rows, activations staged per workgroup in 2048-k chunks, shuffle reduction inside the 32 lanes.  The per-row
//                              order of the sum does not depend on M.
//   2  dense, fast, M > 8      LDS-staged 64 x 128 x 64 tile on v_mfma_f32_32x32x16_bf16 / _f16 (by activation type); the weight bytes are converted to that
//                              type once per workgroup.  A per-scale-block accumulator is folded as total = fma(scale(n, kb), partial, total); n is
//                              the accumulator element's own column, so block_size_y smaller than the tile is correct.
//   3  MoE, fast, <= 8 slots   route 1's kernel, one single-row GEMV per (token, slot), one launch.  Also taken (in launches of 65535 slots) when the slot
//                              list does not fit the LDS.
//   4  MoE, fast, > 8 slots    grid (N tiles, experts): the workgroup gathers its expert's (token, slot) list from `indices` into LDS and runs route 2's body
//                              with indirect row reads and writes.
//   5  general                 everything the fast test declines (K % 16 != 0, block_size_x % 16 != 0, unaligned weight base), dense and MoE: one wave per
//                              output element, byte loads, one partial sum per scale block.  Correct, untuned.
#include "mxfp4_core.cuh"  // unpack2

namespace mrs {

static int g_fp8bw_route = 0;

__device__ __forceinline__ int4 ld16nt_a16(const void *p) { int4_a16 v = __builtin_nontemporal_load((const int4_a16 *)p); return make_int4(v.x, v.y, v.z, v.w); }

// 4 codes of a word -> 4 f32
__device__ __forceinline__ void fp8x4_to_f32(uint32_t q, float *o) {
#if defined(__gfx950__)
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)q, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)q, true);
  o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
#else
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = fp8_e4m3_to_float((uint8_t)(q >> (8 * i)));
#endif
}

// two E4M3 values (as f32) -> two packed T, exact: 4 significand bits and an exponent range both 16-bit types hold
template <class T> __device__ __forceinline__ uint32_t pack2_exact(float a, float b) {
  if constexpr (__is_same(T, bf16_t)) return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xFFFF0000u);
  else return (uint32_t)float_to_half_bits(a) | ((uint32_t)float_to_half_bits(b) << 16);
}

__host__ __device__ __forceinline__ int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------------------------------------ dequantize / quantize
// one workgroup per weight block (tile); 64 lanes along x, 4 waves along y
template <class T>
__global__ void __launch_bounds__(256) fp8_blockwise_dequant_kernel(const uint8_t *__restrict__ w, const float *__restrict__ sc, T *__restrict__ out, int H, int W,
                                                                    int row_stride, int scale_stride, int bsy, int bsx, int gx, long long tiles) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int by = (int)(tile / gx), bx = (int)(tile - (long long)by * gx);
    const float s = sc[(size_t)by * scale_stride + bx];
    const int y1 = min(H, (by + 1) * bsy), x1 = min(W, (bx + 1) * bsx);
    for (int y = by * bsy + ty; y < y1; y += 4)
      for (int x = bx * bsx + tx; x < x1; x += 64) {
        const size_t pos = (size_t)y * row_stride + x;
        float v = fp8_e4m3_to_float(w[pos]) * s;
        asm volatile("" : "+v"(v));  // the f32 product is a value of its own: without this the f16 form becomes one v_fma_mixlo_f16, a single rounding
        out[pos] = from_f<T>(v);
      }
  }
}

template <class T>
__global__ void __launch_bounds__(256) fp8_blockwise_quant_kernel(const T *__restrict__ in, uint8_t *__restrict__ w, float *__restrict__ sc, int H, int W, int row_stride,
                                                                  int scale_stride, int bsy, int bsx, int gx, long long tiles) {
  __shared__ float wave_amax[4];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int by = (int)(tile / gx), bx = (int)(tile - (long long)by * gx);
    const int y0 = by * bsy, x0 = bx * bsx, y1 = min(H, y0 + bsy), x1 = min(W, x0 + bsx);
    float amax = 0.0f;  // over the in-range elements only
    for (int y = y0 + ty; y < y1; y += 4)
      for (int x = x0 + tx; x < x1; x += 64) amax = fmaxf(amax, fabsf(to_f<T>(in[(size_t)y * row_stride + x])));
    amax = wave_max(amax);
    __syncthreads();  // the previous tile's reads of wave_amax are done
    if (tx == 0) wave_amax[ty] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(wave_amax[0], wave_amax[1]), fmaxf(wave_amax[2], wave_amax[3]));
    float s = amax / 448.0f;
    if (s < 1e-12f) s = 1e-12f;
    if (threadIdx.x == 0) sc[(size_t)by * scale_stride + bx] = s;
    for (int y = y0 + ty; y < y1; y += 4)
      for (int x = x0 + tx; x < x1; x += 64) {
        const size_t pos = (size_t)y * row_stride + x;
        float v = to_f<T>(in[pos]) / s;
        if (v > 448.0f) v = 448.0f;
        if (v < -448.0f) v = -448.0f;
        w[pos] = float_to_fp8_e4m3(half_bits_to_float(float_to_half_bits(v)));  // f32 -> f16 -> e4m3: the reference's two roundings
      }
  }
}

// ------------------------------------------------------------------------------------------------ route 1 / 3: streaming GEMV
constexpr int F8_KC = 2048;  // activation elements per row staged at a time
constexpr int F8_ROWS = 8;   // weight rows per 256-thread workgroup (32 lanes each)

// `shift` >= 0: block_size_x == 1 << shift
template <class T, int MR, bool MOE>
__global__ void __launch_bounds__(256) fp8_blockwise_gemv_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, const float *__restrict__ sc,
                                                                 const uint32_t *__restrict__ indices, T *__restrict__ out, int N, int K, int stride, int bsy, int bsx,
                                                                 int shift, int topk, int num_experts, int has_topk_dim, int slot0) {
  __shared__ __attribute__((aligned(16))) T xs[MR * F8_KC];
  if constexpr (MOE) {
    const int slot = slot0 + blockIdx.y;
    const uint32_t e = indices[slot];
    if (e >= (uint32_t)num_experts) return;  // uniform over the workgroup
    x += (size_t)(has_topk_dim ? slot : slot / topk) * K;
    w += (size_t)e * N * K;
    sc += (size_t)e * ceil_div(N, bsy) * stride;
    out += (size_t)slot * N;
  }
  const int tid = threadIdx.x, sub = tid & 31, n = blockIdx.x * F8_ROWS + (tid >> 5);
  const bool live = n < N;
  const uint8_t *wr = w + (size_t)(live ? n : 0) * K;
  const float *sr = sc + (size_t)((live ? n : 0) / bsy) * stride;
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += F8_KC) {
    const int kc = min(F8_KC, K - k0), c8 = kc >> 3;
    __syncthreads();
    for (int i = tid; i < MR * c8; i += 256) {
      const int m = i / c8, c = i - m * c8;
      *(int4 *)(xs + m * F8_KC + c * 8) = ld16_a2(x + (size_t)m * K + k0 + c * 8);
    }
    __syncthreads();
    if (live) {
#pragma unroll 2
      for (int c = sub; c < (kc >> 4); c += 32) {
        const int k = k0 + c * 16;
        const int4 q = ld16nt_a16(wr + k);
        const float s = sr[shift >= 0 ? k >> shift : k / bsx];
        float wv[16];
        fp8x4_to_f32((uint32_t)q.x, wv);
        fp8x4_to_f32((uint32_t)q.y, wv + 4);
        fp8x4_to_f32((uint32_t)q.z, wv + 8);
        fp8x4_to_f32((uint32_t)q.w, wv + 12);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          float p = 0.0f;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int4 xv = *(const int4 *)(xs + m * F8_KC + c * 16 + j * 8);
            float a0, a1;
            unpack2<T>((uint32_t)xv.x, a0, a1); p = fmaf(a0, wv[8 * j + 0], p); p = fmaf(a1, wv[8 * j + 1], p);
            unpack2<T>((uint32_t)xv.y, a0, a1); p = fmaf(a0, wv[8 * j + 2], p); p = fmaf(a1, wv[8 * j + 3], p);
            unpack2<T>((uint32_t)xv.z, a0, a1); p = fmaf(a0, wv[8 * j + 4], p); p = fmaf(a1, wv[8 * j + 5], p);
            unpack2<T>((uint32_t)xv.w, a0, a1); p = fmaf(a0, wv[8 * j + 6], p); p = fmaf(a1, wv[8 * j + 7], p);
          }
          acc[m] = fmaf(s, p, acc[m]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    float v = acc[m];
#pragma unroll
    for (int d = 16; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);  // stays inside the row's 32 lanes
    if (live && sub == 0) out[(size_t)m * N + n] = from_f<T>(v);
  }
}

struct Fp8Geom {
  int stride, bsy, bsx, shift;
};

template <class T, int MR> static void gemv_rows(const T *x, const uint8_t *w, const float *sc, T *out, int N, int K, Fp8Geom g, hipStream_t st) {
  hipLaunchKernelGGL((fp8_blockwise_gemv_kernel<T, MR, false>), dim3(ceil_div(N, F8_ROWS)), dim3(256), 0, st, x, w, sc, (const uint32_t *)nullptr, out, N, K, g.stride,
                     g.bsy, g.bsx, g.shift, 0, 0, 0, 0);
}

template <class T> static void gemv_dense(const T *x, const uint8_t *w, const float *sc, T *out, int M, int N, int K, Fp8Geom g, hipStream_t st) {
  switch (M) {
  case 1: gemv_rows<T, 1>(x, w, sc, out, N, K, g, st); break;
  case 2: gemv_rows<T, 2>(x, w, sc, out, N, K, g, st); break;
  case 3: gemv_rows<T, 3>(x, w, sc, out, N, K, g, st); break;
  case 4: gemv_rows<T, 4>(x, w, sc, out, N, K, g, st); break;
  case 5: gemv_rows<T, 5>(x, w, sc, out, N, K, g, st); break;
  case 6: gemv_rows<T, 6>(x, w, sc, out, N, K, g, st); break;
  case 7: gemv_rows<T, 7>(x, w, sc, out, N, K, g, st); break;
  default: gemv_rows<T, 8>(x, w, sc, out, N, K, g, st); break;
  }
}

// ------------------------------------------------------------------------------------------------ route 2 / 4: 16-bit MFMA tile, scales outside
constexpr int TM = 64, TN = 128, TK = 64;
constexpr int TLD = TK + 8;  // LDS row stride in 16-bit elements (144 B): the 16-byte fragment reads of 32 consecutive rows spread over the banks
typedef __bf16 f8_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f8_f16x8 __attribute__((ext_vector_type(8)));
typedef float f8_f32x16 __attribute__((ext_vector_type(16)));

struct Fp8TileLds {
  uint16_t a[TM * TLD];
  uint16_t b[TN * TLD];
  int count;
};

template <class T> __device__ __forceinline__ f8_f32x16 mfma_32x32x16(const uint16_t *a, const uint16_t *b, f8_f32x16 c) {
  if constexpr (__is_same(T, f16_t)) return __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const f8_f16x8 *)a, *(const f8_f16x8 *)b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const f8_bf16x8 *)a, *(const f8_bf16x8 *)b, c, 0, 0, 0);
}

// 8 codes -> 8 T, packed
template <class T> __device__ __forceinline__ int4 fp8x8_to_t(uint32_t q0, uint32_t q1) {
  float f[8];
  fp8x4_to_f32(q0, f);
  fp8x4_to_f32(q1, f + 4);
  return make_int4((int)pack2_exact<T>(f[0], f[1]), (int)pack2_exact<T>(f[2], f[3]), (int)pack2_exact<T>(f[4], f[5]), (int)pack2_exact<T>(f[6], f[7]));
}

// One TM x TN output tile.  Local row i of the tile is row rows[i] of the output (GATHER: a flat (token, slot) index from the expert's list) or m0 + i.
// A operand = activations [row][k], B operand = unscaled weights [n][k]; lane l of a wave holds k = 8 (l >> 5) + j of row / column l & 31 in element j.
// The accumulator's column (the weight row n) sits on the lane, so a lane needs one scale per scale block of k.
template <class T, bool GATHER>
__device__ __forceinline__ void fp8_blockwise_tile(Fp8TileLds &L, const int *list, const T *__restrict__ x, const uint8_t *__restrict__ w, const float *__restrict__ sc,
                                                   T *__restrict__ out, int m0, int rows, int n0, int N, int K, int stride, int bsy, int bsx, int topk, int has_topk_dim) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  // staging roles: A chunks (row, 8 k) tid and tid + 256; B: weight row tid >> 1, 32 k at 32 (tid & 1)
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
  const int bn = n0 + (tid >> 1), bk = (tid & 1) * 32;
  const bool blive = bn < N;
  const uint8_t *brow = w + (size_t)(blive ? bn : 0) * K;

  int4 ra[2], rb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) ra[i] = (arow[i] && k0 + acol[i] < K) ? ld16_a2(arow[i] + k0 + acol[i]) : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) rb[i] = (blive && k0 + bk + 16 * i < K) ? ld16_a16(brow + k0 + bk + 16 * i) : make_int4(0, 0, 0, 0);
  };

  f8_f32x16 acc[2], part[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = part[i][j] = 0.0f;

  const int col = n0 + wv * 32 + r;
  const float *srow = sc + (size_t)(min(col, N - 1) / bsy) * stride;
  const int steps = bsx >> 4;  // MFMA k steps per scale block
  int left = steps, kb = 0;
  float scur = srow[0];

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += TK) {
    __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) *(int4 *)&L.a[((tid + 256 * i) >> 3) * TLD + acol[i]] = ra[i];
    {
      uint16_t *dst = &L.b[(tid >> 1) * TLD + bk];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        *(int4 *)(dst + 16 * i) = fp8x8_to_t<T>((uint32_t)rb[i].x, (uint32_t)rb[i].y);
        *(int4 *)(dst + 16 * i + 8) = fp8x8_to_t<T>((uint32_t)rb[i].z, (uint32_t)rb[i].w);
      }
    }
    __syncthreads();
    if (k0 + TK < K) fetch(k0 + TK);  // in flight behind the MFMAs
#pragma unroll
    for (int s = 0; s < TK / 16; ++s) {
      if (k0 + 16 * s < K) {  // uniform
        const int kk = 16 * s + 8 * h;
        const uint16_t *fb = &L.b[(wv * 32 + r) * TLD + kk];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) part[mi] = mfma_32x32x16<T>(&L.a[(mi * 32 + r) * TLD + kk], fb, part[mi]);
        if (--left == 0 || k0 + 16 * s + 16 >= K) {  // the scale block (or K) ends here: fold
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
              acc[mi][j] = fmaf(scur, part[mi][j], acc[mi][j]);
              part[mi][j] = 0.0f;
            }
          left = steps;
          ++kb;
          if ((long long)kb * bsx < K) scur = srow[kb];
        }
      }
    }
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  if (col < N) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int lr = m0 + mi * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
        if (lr < rows) {
          int dst = lr;
          if constexpr (GATHER) dst = list[lr];
          out[(size_t)dst * N + col] = from_f<T>(acc[mi][j]);
        }
      }
    }
  }
}

template <class T>
__global__ void __launch_bounds__(256) fp8_blockwise_tile_dense_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, const float *__restrict__ sc, T *__restrict__ out,
                                                                       int M, int N, int K, int stride, int bsy, int bsx) {
  __shared__ __attribute__((aligned(16))) Fp8TileLds L;
  fp8_blockwise_tile<T, false>(L, nullptr, x, w, sc, out, blockIdx.y * TM, M, blockIdx.x * TN, N, K, stride, bsy, bsx, 1, 0);
}

template <class T>
__global__ void __launch_bounds__(256) fp8_blockwise_tile_moe_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, const float *__restrict__ sc,
                                                                     const uint32_t *__restrict__ indices, T *__restrict__ out, int total, int topk, int N, int K, int stride,
                                                                     int bsy, int bsx, int has_topk_dim) {
  __shared__ __attribute__((aligned(16))) Fp8TileLds L;
  extern __shared__ int f8_list[];  // [total]: the flat (token, slot) indices routed to this expert
  const int e = blockIdx.y;
  if (threadIdx.x == 0) L.count = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += 256)
    if (indices[i] == (uint32_t)e) f8_list[atomicAdd(&L.count, 1)] = i;  // any order: a row's arithmetic does not depend on its place in the tile
  __syncthreads();
  const int rows = L.count;
  w += (size_t)e * N * K;
  sc += (size_t)e * ceil_div(N, bsy) * stride;
  for (int m0 = 0; m0 < rows; m0 += TM) fp8_blockwise_tile<T, true>(L, f8_list, x, w, sc, out, m0, rows, blockIdx.x * TN, N, K, stride, bsy, bsx, topk, has_topk_dim);
}

// ------------------------------------------------------------------------------------------------ route 5: general
// one wave per output element: row blockIdx.y + row0 (dense: of x; MoE: the flat (token, slot) index), column 4 blockIdx.x + wave
template <class T, bool MOE>
__global__ void __launch_bounds__(256) fp8_blockwise_general_kernel(const T *__restrict__ x, const uint8_t *__restrict__ w, const float *__restrict__ sc,
                                                                    const uint32_t *__restrict__ indices, T *__restrict__ out, int N, int K, int stride, int bsy, int bsx,
                                                                    int topk, int num_experts, int has_topk_dim, int row0) {
  const int row = row0 + blockIdx.y;
  if constexpr (MOE) {
    const uint32_t e = indices[row];
    if (e >= (uint32_t)num_experts) return;
    x += (size_t)(has_topk_dim ? row : row / topk) * K;
    w += (size_t)e * N * K;
    sc += (size_t)e * ceil_div(N, bsy) * stride;
  } else {
    x += (size_t)row * K;
  }
  out += (size_t)row * N;
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const uint8_t *wr = w + (size_t)n * K;
  const float *sr = sc + (size_t)(n / bsy) * stride;
  float acc = 0.0f;
  for (int kb = 0, ks = 0; ks < K; ++kb, ks += bsx) {
    const int ke = min(K, ks + bsx);
    float p = 0.0f;
    for (int k = ks + lane; k < ke; k += 64) p = fmaf(to_f<T>(x[k]), fp8_e4m3_to_float(wr[k]), p);
    acc = fmaf(sr[kb], p, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) out[n] = from_f<T>(acc);
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

static bool fast_ok(const void *w, int K, int bsx) { return (K & 15) == 0 && (bsx & 15) == 0 && ((uintptr_t)w & 15) == 0; }

static Fp8Geom geom(int stride, int bsy, int bsx) {
  int shift = -1;
  if ((bsx & (bsx - 1)) == 0)
    for (shift = 0; (1 << shift) < bsx; ++shift) {}
  return Fp8Geom{stride, bsy, bsx, shift};
}

static unsigned tile_grid(long long tiles) { return (unsigned)(tiles < 0x7fffffffLL ? tiles : 0x7fffffffLL); }

template <class T>
static void dequant(const uint8_t *w, const float *sc, T *out, int H, int W, int row_stride, int scale_stride, int bsy, int bsx, void *stream) {
  if (H <= 0 || W <= 0 || bsy <= 0 || bsx <= 0) return;
  const int gx = ceil_div(W, bsx);
  const long long tiles = (long long)gx * ceil_div(H, bsy);
  hipLaunchKernelGGL((fp8_blockwise_dequant_kernel<T>), dim3(tile_grid(tiles)), dim3(256), 0, (hipStream_t)stream, w, sc, out, H, W, row_stride, scale_stride, bsy, bsx, gx,
                     tiles);
}

template <class T>
static void quant(const T *in, uint8_t *w, float *sc, int H, int W, int row_stride, int scale_stride, int bsy, int bsx, void *stream) {
  if (H <= 0 || W <= 0 || bsy <= 0 || bsx <= 0) return;
  const int gx = ceil_div(W, bsx);
  const long long tiles = (long long)gx * ceil_div(H, bsy);
  hipLaunchKernelGGL((fp8_blockwise_quant_kernel<T>), dim3(tile_grid(tiles)), dim3(256), 0, (hipStream_t)stream, in, w, sc, H, W, row_stride, scale_stride, bsy, bsx, gx,
                     tiles);
}

template <class T>
static void matmul(const void *input, const uint8_t *weight, const float *scale, void *output, int M, int N, int K, int stride, int bsy, int bsx, void *stream) {
  if (M <= 0 || N <= 0 || K <= 0 || stride <= 0 || bsy <= 0 || bsx <= 0) return;
  const T *x = (const T *)input;
  T *out = (T *)output;
  hipStream_t st = (hipStream_t)stream;
  if (!fast_ok(weight, K, bsx)) {
    g_fp8bw_route = 5;
    for (int r0 = 0; r0 < M; r0 += 65535)  // grid.y limit
      hipLaunchKernelGGL((fp8_blockwise_general_kernel<T, false>), dim3(ceil_div(N, 4), min(65535, M - r0)), dim3(256), 0, st, x, weight, scale, (const uint32_t *)nullptr,
                         out, N, K, stride, bsy, bsx, 0, 0, 0, r0);
  } else if (M <= 8) {
    g_fp8bw_route = 1;
    gemv_dense<T>(x, weight, scale, out, M, N, K, geom(stride, bsy, bsx), st);
  } else {
    g_fp8bw_route = 2;
    hipLaunchKernelGGL((fp8_blockwise_tile_dense_kernel<T>), dim3(ceil_div(N, TN), ceil_div(M, TM)), dim3(256), 0, st, x, weight, scale, out, M, N, K, stride, bsy, bsx);
  }
}

template <class T>
static void moe(const void *input, const uint8_t *weights, const float *scales, const uint32_t *indices, void *output, int num_tokens, int topk, int num_experts, int N, int K,
                int stride, int bsy, int bsx, bool input_has_topk_dim, void *stream) {
  if (num_tokens <= 0 || topk <= 0 || num_experts <= 0 || N <= 0 || K <= 0 || stride <= 0 || bsy <= 0 || bsx <= 0) return;
  const T *x = (const T *)input;
  T *out = (T *)output;
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)num_tokens * topk;
  if (!fast_ok(weights, K, bsx)) {
    g_fp8bw_route = 5;
    for (long long s0 = 0; s0 < total; s0 += 65535)
      hipLaunchKernelGGL((fp8_blockwise_general_kernel<T, true>), dim3(ceil_div(N, 4), (unsigned)((total - s0) < 65535 ? (total - s0) : 65535)), dim3(256), 0, st, x, weights,
                         scales, indices, out, N, K, stride, bsy, bsx, topk, num_experts, (int)input_has_topk_dim, (int)s0);
    return;
  }
  const long long list_bytes = total * 4, budget = (long long)max_lds() - (long long)sizeof(Fp8TileLds) - 64;
  if (total > 8 && list_bytes <= budget && total <= 0x7fffffffLL) {
    g_fp8bw_route = 4;
    if (list_bytes > 16 * 1024) lds_attr_once((const void *)fp8_blockwise_tile_moe_kernel<T>, (int)budget);
    hipLaunchKernelGGL((fp8_blockwise_tile_moe_kernel<T>), dim3(ceil_div(N, TN), num_experts), dim3(256), (size_t)list_bytes, st, x, weights, scales, indices, out, (int)total,
                       topk, N, K, stride, bsy, bsx, (int)input_has_topk_dim);
    return;
  }
  g_fp8bw_route = 3;
  const Fp8Geom g = geom(stride, bsy, bsx);
  for (long long s0 = 0; s0 < total; s0 += 65535)  // grid.y limit
    hipLaunchKernelGGL((fp8_blockwise_gemv_kernel<T, 1, true>), dim3(ceil_div(N, F8_ROWS), (unsigned)((total - s0) < 65535 ? (total - s0) : 65535)), dim3(256), 0, st, x,
                       weights, scales, indices, out, N, K, g.stride, g.bsy, g.bsx, g.shift, topk, num_experts, (int)input_has_topk_dim, (int)s0);
}

}  // namespace mrs

extern "C" {

#define MRS_FP8BW_DEQUANT(tag, T)                                                                                                                                   \
  void launch_dequant_fp8_blockwise_kernel_##tag(const uint8_t *d_weight, const float *d_scale, void *d_output, int weight_height, int weight_width,                 \
                                                 int weight_row_stride, int scale_stride, int weight_block_size_y, int weight_block_size_x, void *stream) {          \
    mrs::dequant<T>(d_weight, d_scale, (T *)d_output, weight_height, weight_width, weight_row_stride, scale_stride, weight_block_size_y, weight_block_size_x, stream); \
  }                                                                                                                                                                   \
  void launch_quant_fp8_blockwise_kernel_##tag(const void *d_input, uint8_t *d_weight, float *d_scale, int weight_height, int weight_width, int weight_row_stride,   \
                                               int scale_stride, int weight_block_size_y, int weight_block_size_x, void *stream) {                                  \
    mrs::quant<T>((const T *)d_input, d_weight, d_scale, weight_height, weight_width, weight_row_stride, scale_stride, weight_block_size_y, weight_block_size_x,      \
                  stream);                                                                                                                                            \
  }
MRS_FP8BW_DEQUANT(f32, float)
MRS_FP8BW_DEQUANT(f16, mrs::f16_t)
MRS_FP8BW_DEQUANT(bf16, mrs::bf16_t)
#undef MRS_FP8BW_DEQUANT

#define MRS_FP8BW_MATMUL(tag, T)                                                                                                                                  \
  void launch_fp8_matmul_##tag(const void *input, const uint8_t *weight, const float *weight_scale, void *output, int M, int N, int K, int scale_row_stride,       \
                               int block_size_y, int block_size_x, void *stream) {                                                                                 \
    mrs::matmul<T>(input, weight, weight_scale, output, M, N, K, scale_row_stride, block_size_y, block_size_x, stream);                                            \
  }                                                                                                                                                                 \
  void launch_fp8_indexed_moe_gemm_##tag(const void *input, const uint8_t *weights, const float *weight_scales, const uint32_t *indices, void *output,              \
                                         int num_tokens, int topk, int num_experts, int N, int K, int scale_row_stride, int block_size_y, int block_size_x,        \
                                         bool input_has_topk_dim, void *stream) {                                                                                   \
    mrs::moe<T>(input, weights, weight_scales, indices, output, num_tokens, topk, num_experts, N, K, scale_row_stride, block_size_y, block_size_x,                  \
                input_has_topk_dim, stream);                                                                                                                        \
  }
MRS_FP8BW_MATMUL(f16, mrs::f16_t)
MRS_FP8BW_MATMUL(bf16, mrs::bf16_t)
#undef MRS_FP8BW_MATMUL

int fp8_blockwise_last_route(void) { return mrs::g_fp8bw_route; }

}  // extern "C"
