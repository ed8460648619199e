// dec_epilogue.cuh -- what a linear of the decode engine does with a finished row, written ONCE for every kernel that can produce the row: the vector-ALU GEMV
// (dec_gemv.cuh), the matrix-core kernel (ext_dec_mm.hip) and the exact prompt path (ext_gemm_qi.hip).  "A token's bits do not depend on the kernel that produced
// them" is these expressions; a kernel keeps only what is its own -- how a lane finds its RoPE partner, which lanes write, when the RoPE factors are loaded.
//
// Rules of this header (dec_core2.cuh and ext_dec_mm.hip document how easily hipcc sends these kernels to scratch memory): plain __device__ __forceinline__
// functions, operands by value (scalars, small PODs), no by-reference lambda of a kernel, and nothing here takes the address of -- or selects between addresses
// inside -- a kernel's argument block.
#pragma once
#include "common.cuh"

namespace mrs {
namespace dec {

// RESID: out = old * rs + sum * w -- two products and one add, three roundings.  Every build of these sources compiles with -ffp-contract=off (build.py,
// oracle/build_hip_host.sh): no fused multiply-add forms here, on any route.
__device__ __forceinline__ float resid_fold(float old, float rs, float sum, float w) { return old * rs + sum * w; }

// GLU: act(gate) * up; activation 0 = SiLU through the engine's exponential, else the codes of glu_act
__device__ __forceinline__ float glu_value(float g, float u, int activation) { return (activation == 0 ? silu_engine(g) : glu_act(g, activation)) * u; }

// ------------------------------------------------------------------------------------------------ q / k / v: RoPE + q store + paged K / V write
// Rows 2i, 2i + 1 of a tensor are a RoPE pair (tensor 0 = q, 1 = k, 2 = v: never rotated).  The cache is the reference's paged layout: K [blocks][kv heads]
// [head_dim / x][block_size][x], V [blocks][kv heads][head_dim][block_size]; 16-bit elements with x = 8, or -- kv_fp8 -- FP8 E4M3 bytes with x = 16 and one static
// scale per tensor: code = float_to_fp8_e4m3(value / scale), the expression of kv_cache_ops.hip conv<float, fp8_t> (reshape_and_cache writes the same byte).
struct QkvEpi {
  float *q_out; void *k_cache, *v_cache; const int64_t *slot_mapping; const int32_t *positions; const float *cos_t, *sin_t;
  int head_dim, rot_pairs, num_kv_heads, block_size, cache_x, kv_f16;
  int kv_fp8; float k_scale, v_scale;  // FP8 pages (qkv_store_f8)
  int hd_shift, bs_shift, x_shift;  // log2 of head_dim / block_size / cache_x (qkv_epi_fill refuses other values): the index arithmetic is shifts and masks -- with
                                    // run-time divisors it was ~10 integer divisions per column and row pair (~40 VALU each), 10 us of the batch-8 qkv launch
};

// the RoPE factors of local row `row` of tensor ti at position pos: identity for v and for unrotated dims (x * 1 - y * 0 = x exactly).  Unconditional loads from a
// clamped index: a lane-conditional load is a branch around a VMEM instruction (dec_core2.cuh stream()).
struct RopeCS { float c, s; };
__device__ __forceinline__ RopeCS qkv_rope_factors(const QkvEpi e, int ti, int pos, int row) {
  const int pair_i = (row & (e.head_dim - 1)) >> 1;
  const bool rot = ti < 2 && pair_i < e.rot_pairs;
  const int pi = min(pair_i, e.rot_pairs - 1);
  const size_t tix = (size_t)pos * e.rot_pairs + pi;
  const float cs = e.cos_t[tix], sn = e.sin_t[tix];
  return RopeCS{rot ? cs : 1.0f, rot ? sn : 0.0f};
}

// where the two results of the pair with even local row lr live: adjacent dims (interleaved RoPE), or dims i and i + head_dim / 2 when the rows of q / k were stored
// in pair order (neox; v: never)
struct QkvDst { int head, dd, d0, d1; };
__device__ __forceinline__ QkvDst qkv_dst(const QkvEpi e, int ti, int neox, int lr) {
  const int head = lr >> e.hd_shift, dd = lr & (e.head_dim - 1);
  const bool nx = neox && ti < 2;
  const int d0 = nx ? dd >> 1 : dd, d1 = nx ? d0 + (e.head_dim >> 1) : dd + 1;
  return QkvDst{head, dd, d0, d1};
}

__device__ __forceinline__ uint16_t kv_bits(int kv_f16, float v) { return kv_f16 ? float_to_half_bits(v) : float_to_bf16_bits(v); }
// element index of dim d of (head base hb, in-page offset off) in the K pages
__device__ __forceinline__ size_t k_page_index(const QkvEpi e, size_t hb, unsigned off, int d) {
  const int X = e.cache_x;
  return (hb + ((unsigned)d >> e.x_shift)) * e.block_size * X + off * X + ((unsigned)d & (unsigned)(X - 1));
}

// the k / v half of qkv_store for FP8 pages: byte stores, same index arithmetic (cache_x = 16)
__device__ __forceinline__ void qkv_store_f8(const QkvEpi e, int ti, unsigned blk, unsigned off, const QkvDst t, float x, float y, bool wr0, bool wr1) {
  uint8_t *kc = (uint8_t *)e.k_cache, *vc = (uint8_t *)e.v_cache;
  const float sc = ti == 1 ? e.k_scale : e.v_scale;
  const uint8_t xb = float_to_fp8_e4m3(x / sc), yb = float_to_fp8_e4m3(y / sc);
  if (ti == 1) {
    const size_t hb = ((size_t)blk * e.num_kv_heads + t.head) * (size_t)(e.head_dim >> e.x_shift);
    if (wr0) kc[k_page_index(e, hb, off, t.d0)] = xb;
    if (wr1) kc[k_page_index(e, hb, off, t.d1)] = yb;
  } else {
    const size_t o = (((size_t)blk * e.num_kv_heads + t.head) * e.head_dim + t.dd) * e.block_size + off;
    if (wr0) vc[o] = xb;
    if (wr1) vc[o + e.block_size] = yb;
  }
}

// store the rotated pair (x -> d0 when wr0, y -> d1 when wr1) of column c: q_out [c][nq] for q, the page of `slot` for k / v (slot < 0: a padded sequence, nothing).
// F8: 0 / 1 = the page format is the kernel's compile-time property (the vector-ALU GEMV: its 16-bit instantiations carry no FP8 code and compile as they did before
// FP8 pages; profiles/fp8_kv.md has the bench runs of both forms), -1 = decided per launch by e.kv_fp8 (the matrix-core kernel).
template <int F8 = -1>
__device__ __forceinline__ void qkv_store(const QkvEpi e, int ti, int nq, int c, int slot, const QkvDst t, float x, float y, bool wr0, bool wr1) {
  if (ti == 0) {
    if (wr0) e.q_out[(size_t)c * nq + t.head * e.head_dim + t.d0] = x;
    if (wr1) e.q_out[(size_t)c * nq + t.head * e.head_dim + t.d1] = y;
  } else if (slot >= 0) {
    const unsigned blk = (unsigned)slot >> e.bs_shift, off = (unsigned)slot & (unsigned)(e.block_size - 1);
    if (F8 < 0 ? e.kv_fp8 != 0 : F8 != 0) { qkv_store_f8(e, ti, blk, off, t, x, y, wr0, wr1); return; }  // launch-uniform or compile-time
    uint16_t *kc = (uint16_t *)e.k_cache, *vc = (uint16_t *)e.v_cache;
    const uint16_t xb = kv_bits(e.kv_f16, x), yb = kv_bits(e.kv_f16, y);
    if (ti == 1) {
      const size_t hb = ((size_t)blk * e.num_kv_heads + t.head) * (size_t)(e.head_dim >> e.x_shift);
      if (wr0) kc[k_page_index(e, hb, off, t.d0)] = xb;
      if (wr1) kc[k_page_index(e, hb, off, t.d1)] = yb;
    } else {
      const size_t o = (((size_t)blk * e.num_kv_heads + t.head) * e.head_dim + t.dd) * e.block_size + off;
      if (wr0) vc[o] = xb;
      if (wr1) vc[o + e.block_size] = yb;
    }
  }
}

// a static FP8 page scale an entry point accepts: finite and > 0
inline bool kv_scale_ok(float s) { return s > 0.f && s < __builtin_inff(); }

// host: fill and validate the block for a launch of n_q / n_k / n_v rows (kv_dtype 1 = bf16, 0 = f16; 3 = FP8 E4M3 with k_scale / v_scale finite and > 0, which only
// the *_f8 entry points pass).  False = the epilogue cannot index this shape: odd row counts
// or head size, sizes that are not powers of two (every head size the engine's attention takes, every block size of the reference's cache), no rotated pair (the
// factor lookup clamps to rot_pairs - 1).
inline bool qkv_epi_fill(QkvEpi &e, float *q_out, void *k_cache, void *v_cache, const int64_t *slot_mapping, const int32_t *positions, const float *cos_t,
                         const float *sin_t, int head_dim, int rot_pairs, int num_kv_heads, int block_size, int kv_dtype, long long n_q, long long n_k, long long n_v,
                         float k_scale = 0.f, float v_scale = 0.f) {
  const bool f8 = kv_dtype == 3;
  if (((n_q | n_k | n_v | head_dim) & 1) || (kv_dtype != 0 && kv_dtype != 1 && !f8) || rot_pairs < 1) return false;
  if (f8 && !(kv_scale_ok(k_scale) && kv_scale_ok(v_scale))) return false;
  auto lg2 = [](int v) { int s = 0; while (s < 30 && (1 << s) < v) ++s; return (1 << s) == v ? s : -1; };
  e.q_out = q_out; e.k_cache = k_cache; e.v_cache = v_cache; e.slot_mapping = slot_mapping; e.positions = positions; e.cos_t = cos_t; e.sin_t = sin_t;
  e.head_dim = head_dim; e.rot_pairs = rot_pairs; e.num_kv_heads = num_kv_heads; e.block_size = block_size; e.cache_x = f8 ? 16 : 8; e.kv_f16 = kv_dtype == 0;
  e.kv_fp8 = f8; e.k_scale = k_scale; e.v_scale = v_scale;
  e.hd_shift = lg2(head_dim); e.bs_shift = lg2(block_size); e.x_shift = lg2(e.cache_x);
  return e.hd_shift >= 0 && e.bs_shift >= 0 && head_dim >= e.cache_x;
}

}  // namespace dec
}  // namespace mrs
