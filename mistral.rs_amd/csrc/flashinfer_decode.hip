// flashinfer_decode.hip -- GQA decode attention over an HND paged cache, request lists in CSR form, split-KV by a device-side tile plan; the two cache
// ops of that layout.  gfx950 matrix cores.
//
// Role in the reference: `reshape_and_cache_flashinfer`, `gather_kv_cache_flashinfer` and `flashinfer_decode` of mistralrs-paged-attn/src/cuda/
// flashinfer_decode.cu (callers backend/flashinfer.rs, plan mistralrs-core/src/flashinfer/metadata.rs).  Semantics:
//   key_cache / value_cache [num_pages, kv_heads, page_size, head_size]  (HND; element = query dtype or E4M3 holding value / scale)
//   len_b = (indptr[b + 1] - indptr[b] - 1) * page_size + last_page_len[b] (0 without a page); key i lives in page indices[indptr[b] + i / page_size]
//   workgroup (bx, kv head): nothing when block_valid_mask[bx] == 0; else request b = request_indices[bx], plan tile t = kv_tile_indices[bx], keys
//   [t chunk, min((t + 1) chunk, len_b)) with chunk = *kv_chunk_size_ptr, or all of [0, len_b) when tmp_v == NULL
//   s_i = sm_scale k_scale (q . k_i), with a cap s_i = cap tanh(s_i / cap); key i is visible iff window_left < 0 or i + 1 + window_left >= len_b
//   o = v_scale softmax_visible(s) . v (zeros without a visible key)
//
// MI355X design.  A workgroup of four waves serves the G = heads / kv_heads query heads of one KV head over one plan tile, on
// v_mfma_f32_16x16x32_{bf16,f16}: 16 keys x 16 heads per instruction, so all of a tile is useful at G = 16 (the 32x32x16 form would idle half of it).
// The plan tile is cut into 32-key tiles and wave w takes tiles w, w + 4, ...: no wave waits for another inside the loop.  Per tile a wave
//   * holds K in registers only: lane (key n = lane & 15, g = lane >> 4) loads 16 bytes of key row 16 mb + n per k-step -- in an HND page those are the 8
//     consecutive dims of the A fragment of S^T = K Q^T.  Q^T (heads zero-padded to 16) is the B fragment, loaded once, resident for the whole loop.
//     An E4M3 row is loaded 16 bytes = 16 dims at a time and feeds two k-steps; the dims of a k-step are then 64 (ks / 2) + 16 g + 8 (ks & 1) + 0..7,
//     and Q is loaded in the same order.  Codes are widened to the query dtype in registers (v_cvt_pk_f32_fp8, exact) just before the MFMA;
//   * turns V through its own LDS region: lane (key pair p = lane >> 2, chunk c4 = lane & 3) loads the same 8 dims of keys 2p and 2p + 1 and writes 8
//     words [dim][p] = (V[2p][dim], V[2p + 1][dim]), rows of V_ROW = 20 words.  The A fragment of O^T = V^T P^T -- lane = (dim n, g), keys 4g .. 4g + 3
//     and 16 + 4g .. + 3 -- is two ds_read_b64.  20 n mod 64 are 16 different multiples of 4, so the 32 lanes of a half wave read 32 different bank pairs;
//     a wave's 64 one-word writes land in banks 32 (c4 & 1) + 20 j + p, and lanes with c4 >= 2 write their 8 words rotated by 4 (20 * 4 = 16 mod 64),
//     which makes the four chunks disjoint runs of 16 banks;
//   * S^T leaves a lane with 8 keys of ONE head (lane & 15), the head whose column of O^T it also holds: scale, cap, mask, running max and sum are register
//     math plus two exchanges (lane ^ 16, lane ^ 32), and P, rounded once to the tensor dtype, is in place the B fragment of the second product (the
//     order of keys inside the 32-key k-dimension is free as long as V^T is read in the same order);
//   * rows >= the tile's end are zeros, never loaded (an unwritten row may hold NaN, and 0 * NaN poisons an MFMA), heads >= G are zero Q fragments;
//   * the loads of the wave's next tile are issued as soon as the registers are free (V after its LDS write, K after the S^T MFMAs), and the page ids
//     of the tile after that right behind them.
// 32-key tiles wholly before the window are skipped (the loop starts at the window).  After the loop the four (m, l, O) states meet in LDS once, are
// merged in wave order, and either the output row or -- with tmp_v -- the normalised f32 partial and its log-sum-exp are written; a second small launch
// merges a request's partials in index order.
#include "common.cuh"
#include "mistralrs_paged_attn.h"
#include <float.h>
#include <math.h>
#include <stdio.h>

namespace mrs {
namespace fid {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

template <class T> struct Mma;
template <> struct Mma<bf16_t> {
  static __device__ __forceinline__ f32x4 run(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ unsigned pk(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  }
};
template <> struct Mma<f16_t> {
  static __device__ __forceinline__ f32x4 run(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ unsigned pk(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
  }
};

// 8 E4M3 codes -> 8 values of T, exact: every E4M3 value is an f16 and a bf16
template <class T> __device__ __forceinline__ uint4 widen8(unsigned lo4, unsigned hi4) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo4, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo4, true);
  const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi4, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi4, true);
  return make_uint4(Mma<T>::pk(a[0], a[1]), Mma<T>::pk(b[0], b[1]), Mma<T>::pk(c[0], c[1]), Mma<T>::pk(d[0], d[1]));
}

static void check_launch(const char *what) {  // a launch error ends the process, like the reference's CUDA_CHECK
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "%s: launch failed: %s\n", what, hipGetErrorString(e));
    abort();
  }
}

// ---------------------------------------------------------------------------------- cache ops
// One workgroup per token, K then V.  A lane moves 16 bytes of the dense side (EPC elements: one head never straddles a piece when head_size % EPC == 0)
// when both ends are aligned for it, single elements otherwise.  E4M3 pages hold value / scale and give back float(code) * scale.
template <class T, bool F8> __device__ __forceinline__ void put(void *cache, int64_t o, T x, float scale) {
  if constexpr (F8) ((uint8_t *)cache)[o] = float_to_fp8_e4m3(to_f<T>(x) / scale);
  else ((T *)cache)[o] = x;
}
template <class T, bool F8> __device__ __forceinline__ T get(const void *cache, int64_t o, float scale) {
  if constexpr (F8) return from_f<T>(fp8_e4m3_to_float(((const uint8_t *)cache)[o]) * scale);
  else return ((const T *)cache)[o];
}

template <class T, bool F8>
__global__ void __launch_bounds__(256) reshape_and_cache_kernel(const T *key, const T *value, void *key_cache, void *value_cache, const int64_t *slot_mapping,
                                                                int H, int D, int bs, int key_stride, int value_stride, float k_scale, float v_scale) {
  constexpr int EPC = 16 / (int)sizeof(T), CB = F8 ? EPC : 16;  // elements and cache bytes of a piece
  const int64_t tok = blockIdx.x, slot = slot_mapping[tok];
  if (slot < 0) return;  // padding token
  const int64_t row0 = slot / bs * H * bs + slot % bs;  // cache row of head 0; head h is h * bs rows further
#pragma unroll
  for (int kv = 0; kv < 2; ++kv) {
    const T *src = kv ? value + tok * value_stride : key + tok * key_stride;
    void *cache = kv ? value_cache : key_cache;
    const float scale = kv ? v_scale : k_scale;
    const int n = H * D;
    int done = 0;
    if (D % EPC == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)cache & (CB - 1)) == 0) {
      for (int i = threadIdx.x; i < n / EPC; i += blockDim.x) {
        const int e = i * EPC;
        const int64_t o = (row0 + (int64_t)(e / D) * bs) * D + e % D;
        const uint4 x = *(const uint4 *)(src + e);
        if constexpr (!F8) {
          *(uint4 *)((T *)cache + o) = x;
        } else {
          T v[EPC];
          __builtin_memcpy(v, &x, 16);
          uint8_t c[EPC];
#pragma unroll
          for (int j = 0; j < EPC; ++j) c[j] = float_to_fp8_e4m3(to_f<T>(v[j]) / scale);
          if constexpr (EPC == 8) { uint2 w; __builtin_memcpy(&w, c, 8); *(uint2 *)((uint8_t *)cache + o) = w; }
          else { unsigned w; __builtin_memcpy(&w, c, 4); *(unsigned *)((uint8_t *)cache + o) = w; }
        }
      }
      done = n;
    }
    for (int e = done + threadIdx.x; e < n; e += blockDim.x) put<T, F8>(cache, (row0 + (int64_t)(e / D) * bs) * D + e % D, src[e], scale);
  }
}

template <class T, bool F8>
__global__ void __launch_bounds__(256) gather_kernel(const void *key_cache, const void *value_cache, T *k_out, T *v_out, const int *block_table,
                                                     const int *cu_seq_lens, int num_seqs, int bs, int block_table_stride, int H, int D, float k_scale,
                                                     float v_scale) {
  constexpr int EPC = 16 / (int)sizeof(T), CB = F8 ? EPC : 16;
  const int tok = blockIdx.x;
  int lo = 0, hi = num_seqs - 1;  // the last sequence with cu_seq_lens[s] <= tok (empty sequences before it are passed over)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cu_seq_lens[mid] <= tok) lo = mid; else hi = mid - 1;
  }
  const int pos = tok - cu_seq_lens[lo];
  const int64_t row0 = (int64_t)block_table[(int64_t)lo * block_table_stride + pos / bs] * H * bs + pos % bs;
#pragma unroll
  for (int kv = 0; kv < 2; ++kv) {
    const void *cache = kv ? value_cache : key_cache;
    T *dst = (kv ? v_out : k_out) + (int64_t)tok * H * D;
    const float scale = kv ? v_scale : k_scale;
    const int n = H * D;
    int done = 0;
    if (D % EPC == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)cache & (CB - 1)) == 0) {
      for (int i = threadIdx.x; i < n / EPC; i += blockDim.x) {
        const int e = i * EPC;
        const int64_t o = (row0 + (int64_t)(e / D) * bs) * D + e % D;
        uint4 x;
        if constexpr (!F8) {
          x = *(const uint4 *)((const T *)cache + o);
        } else {
          uint8_t c[EPC];
          if constexpr (EPC == 8) { const uint2 w = *(const uint2 *)((const uint8_t *)cache + o); __builtin_memcpy(c, &w, 8); }
          else { const unsigned w = *(const unsigned *)((const uint8_t *)cache + o); __builtin_memcpy(c, &w, 4); }
          T v[EPC];
#pragma unroll
          for (int j = 0; j < EPC; ++j) v[j] = from_f<T>(fp8_e4m3_to_float(c[j]) * scale);
          __builtin_memcpy(&x, v, 16);
        }
        *(uint4 *)(dst + e) = x;
      }
      done = n;
    }
    for (int e = done + threadIdx.x; e < n; e += blockDim.x) dst[e] = get<T, F8>(cache, (row0 + (int64_t)(e / D) * bs) * D + e % D, scale);
  }
}

// ---------------------------------------------------------------------------------- decode
struct Args {
  const uint16_t *q;
  const void *kc, *vc;
  const int *indptr, *indices, *last, *req, *tile, *o_indptr, *chunk;
  const uint8_t *mask;
  void *o;
  float *tmp_v, *tmp_s;  // [plan tiles, heads, D] normalised partials and [plan tiles, heads] log-sum-exp (-inf: empty); NULL: no partition
  float scale, v_scale, cap;  // scale = sm_scale * k_scale
  int H, Hkv, G, page_shift, window_left;
  int64_t q_stride_n, q_stride_h;
};

constexpr int KT = 32;      // keys per tile
constexpr int V_ROW = 20;   // words of a transposed V row: 16 key pairs + 4 pad
template <int D> struct Lds {
  static constexpr int STAGE = D * V_ROW * 4;  // bytes per wave: the transposed V tile, later the wave's O^T (D * 16 floats)
  static constexpr int ML_OFF = 4 * STAGE;     // [4 waves][16 heads] (m, l)
  static constexpr int BYTES = ML_OFF + 4 * 16 * 2 * 4;
};
static_assert(Lds<256>::BYTES <= LDS_DYN_MAX, "the D = 256 kernel must fit the CU's LDS");

template <class T, bool F8, int D, bool CAP>
__global__ void __launch_bounds__(256) decode_kernel(const Args a) {
  constexpr int KS = D / 32, NDB = D / 16, VC = D / 32;  // k-steps of S^T, 16-dim blocks of O^T, 8-dim V chunks per lane
  constexpr int KR = F8 ? KS / 2 : KS;                   // 16-byte K registers per key row
  constexpr int EB = F8 ? 1 : 2;                         // bytes per cache element
  using L = Lds<D>;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int bx = blockIdx.x, kvh = blockIdx.y;
  if (a.mask[bx] == 0) return;  // a padding entry of the plan: no request is touched
  const int b = a.req[bx], t = a.tile[bx];
  const bool part = a.tmp_v != nullptr;
  if (!part && t != 0) return;  // without a partition the first tile of a request covers all of it
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
  unsigned *vst = (unsigned *)(smem + wave * L::STAGE);
  float *mls = (float *)(smem + L::ML_OFF);

  const int ip0 = a.indptr[b], npages = a.indptr[b + 1] - ip0;
  const int len = npages > 0 ? ((npages - 1) << a.page_shift) + a.last[b] : 0;
  int kbeg = 0, kend = len;
  if (part) {
    const int64_t chunk = *a.chunk;  // a multiple of the page size (the plan's split_pages * page_size)
    kbeg = (int)min((int64_t)len, t * chunk);
    kend = (int)min((int64_t)len, (t + 1) * chunk);
  }
  const int wstart = a.window_left >= 0 ? max(0, len - 1 - a.window_left) : 0;  // the first visible key
  if (wstart > kbeg) kbeg += (wstart - kbeg) / KT * KT;                         // whole tiles before the window are never loaded
  const int pmask = (1 << a.page_shift) - 1;

  // ---- Q^T fragments (B operand: lane = head n, 8 dims of k-step ks), resident for the whole key loop; heads >= G are zeros
  uint4 qf[KS];
  {
    const bool hok = n < a.G;
    const uint16_t *qp = a.q + b * a.q_stride_n + (int64_t)(kvh * a.G + (hok ? n : 0)) * a.q_stride_h;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = F8 ? 64 * (ks >> 1) + 16 * g + 8 * (ks & 1) : 32 * ks + 8 * g;
      int4 v = make_int4(0, 0, 0, 0);
      if (hok) v = ld16_a2(qp + d0);  // q rows need not be 16-byte aligned
      qf[ks] = make_uint4(v.x, v.y, v.z, v.w);
    }
  }
  f32x4 acc[NDB];  // O^T: lane = head n, dims 16 db + 4 g + 0..3
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -FLT_MAX, l = 0.f;

  // ---- loads: K lane = (key row 16 mb + n, g), V lane = (key pair p, chunk c4); both keys of a pair share a page (tiles start on even keys)
  const int p = lane >> 2, c4 = lane & 3;
  uint4 kreg[2][KR];
  uint4 vreg[F8 ? VC : 2 * VC];  // F8: (x, y) = 8 codes of key 2p, (z, w) = 8 codes of key 2p + 1
  int pgk[2] = {0, 0}, pgv = 0;  // page ids of the NEXT load
  auto pages = [&](int t0) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) pgk[mb] = t0 + 16 * mb + n < kend ? a.indices[ip0 + ((t0 + 16 * mb + n) >> a.page_shift)] : 0;
    pgv = t0 + 2 * p < kend ? a.indices[ip0 + ((t0 + 2 * p) >> a.page_shift)] : 0;
  };
  auto row = [&](const void *cache, int page, int key) {  // first byte of a key row of this KV head
    return (const uint8_t *)cache + ((((int64_t)page * a.Hkv + kvh) << a.page_shift) + (key & pmask)) * (D * EB);
  };
  auto load_k = [&](int t0) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int key = t0 + 16 * mb + n;
      const uint8_t *kp = row(a.kc, pgk[mb], key) + 16 * g;
#pragma unroll
      for (int r = 0; r < KR; ++r) kreg[mb][r] = key < kend ? *(const uint4 *)(kp + 64 * r) : make_uint4(0, 0, 0, 0);
    }
  };
  auto load_v = [&](int t0) {
    const int k0 = t0 + 2 * p;
    const uint8_t *vp = row(a.vc, pgv, k0) + 8 * EB * c4;
#pragma unroll
    for (int i = 0; i < VC; ++i) {
      if constexpr (F8) {
        const uint2 e = k0 < kend ? *(const uint2 *)(vp + 32 * i) : make_uint2(0, 0);
        const uint2 f = k0 + 1 < kend ? *(const uint2 *)(vp + D + 32 * i) : make_uint2(0, 0);
        vreg[i] = make_uint4(e.x, e.y, f.x, f.y);
      } else {
        vreg[2 * i] = k0 < kend ? *(const uint4 *)(vp + 64 * i) : make_uint4(0, 0, 0, 0);
        vreg[2 * i + 1] = k0 + 1 < kend ? *(const uint4 *)(vp + 2 * D + 64 * i) : make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto store_v = [&]() {  // transposed: word [dim][p] = (V[2p][dim], V[2p + 1][dim]); lanes with c4 >= 2 write their 8 words rotated by 4
    const bool rot = c4 >= 2;
#pragma unroll
    for (int i = 0; i < VC; ++i) {
      uint4 e, f;
      if constexpr (F8) {
        e = widen8<T>(vreg[i].x, vreg[i].y);
        f = widen8<T>(vreg[i].z, vreg[i].w);
      } else {
        e = vreg[2 * i];
        f = vreg[2 * i + 1];
      }
      const unsigned ew[4] = {e.x, e.y, e.z, e.w}, fw[4] = {f.x, f.y, f.z, f.w};
      unsigned w[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[2 * j] = (ew[j] & 0xffffu) | (fw[j] << 16);
        w[2 * j + 1] = (ew[j] >> 16) | (fw[j] & 0xffff0000u);
      }
      unsigned *vt = vst + (8 * (4 * i + c4)) * V_ROW + p;
#pragma unroll
      for (int s = 0; s < 8; ++s) vt[(rot ? (s + 4) & 7 : s) * V_ROW] = rot ? w[(s + 4) & 7] : w[s];
    }
  };

  const int tfirst = kbeg + wave * KT;
  if (tfirst < kend) {
    pages(tfirst);
    load_k(tfirst);
    load_v(tfirst);
    pages(tfirst + 4 * KT);
  }
  for (int t0 = tfirst; t0 < kend; t0 += 4 * KT) {
    const int tn = t0 + 4 * KT;  // this wave's next tile
    MRS_WAVE_SYNC();  // the wave's reads of its previous tile are issued before the region is overwritten
    store_v();
    MRS_WAVE_SYNC();
    if (tn < kend) load_v(tn);
    // ---- S^T = K Q^T: 32 keys x 16 heads over D dims
    f32x4 sacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        uint4 af;
        if constexpr (F8) {
          const uint4 raw = kreg[mb][ks >> 1];
          af = (ks & 1) ? widen8<T>(raw.z, raw.w) : widen8<T>(raw.x, raw.y);
        } else {
          af = kreg[mb][ks];
        }
        sacc[mb] = Mma<T>::run(af, qf[ks], sacc[mb]);
      }
    if (tn < kend) {
      load_k(tn);
      pages(tn + 4 * KT);
    }
    // ---- online softmax of head n: this lane holds keys 16 mb + 4 g + j of the tile
    float sv[8], mx = -FLT_MAX;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int kpos = t0 + 16 * (r >> 2) + 4 * g + (r & 3);
      float x = sacc[r >> 2][r & 3] * a.scale;
      if constexpr (CAP) x = a.cap * tanhf(x / a.cap);
      sv[r] = kpos < kend && kpos >= wstart ? x : -FLT_MAX;
      mx = fmaxf(mx, sv[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    const float alpha = __expf(m - mn);
    float pr[8], ps = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      pr[r] = sv[r] > -FLT_MAX ? __expf(sv[r] - mn) : 0.f;
      ps += pr[r];
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
    // ---- O^T += V^T P^T: P is the score registers in place, rounded once to the tensor dtype
    const uint4 pf = make_uint4(Mma<T>::pk(pr[0], pr[1]), Mma<T>::pk(pr[2], pr[3]), Mma<T>::pk(pr[4], pr[5]), Mma<T>::pk(pr[6], pr[7]));
    const unsigned *vp = vst + n * V_ROW + 2 * g;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const uint2 v0 = *(const uint2 *)(vp + 16 * db * V_ROW), v1 = *(const uint2 *)(vp + 16 * db * V_ROW + 8);
      acc[db] = Mma<T>::run(make_uint4(v0.x, v0.y, v1.x, v1.y), pf, acc[db] * alpha);
    }
  }

  // ---- the four waves' states meet once: O^T into each wave's own region, (m, l) next to them, merged in wave order
  MRS_WAVE_SYNC();
  float *ost = (float *)smem;
#pragma unroll
  for (int db = 0; db < NDB; ++db) *(f32x4 *)(ost + wave * (L::STAGE / 4) + (db * 64 + lane) * 4) = acc[db];
  if (g == 0) {
    mls[(wave * 16 + n) * 2] = m;
    mls[(wave * 16 + n) * 2 + 1] = l;
  }
  __syncthreads();
  float M = -FLT_MAX, wgt[4], Lsum = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) M = fmaxf(M, mls[(w * 16 + n) * 2]);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    wgt[w] = __expf(mls[(w * 16 + n) * 2] - M);
    Lsum += wgt[w] * mls[(w * 16 + n) * 2 + 1];
  }
  if (n >= a.G) return;  // padded heads are never stored
  const int head = kvh * a.G + n;
  const int64_t prow = part ? ((int64_t)a.o_indptr[b] + t) * a.H + head : 0;
  const float inv = Lsum > 0.f ? (part ? 1.f : a.v_scale) / Lsum : 0.f;
  if (part && wave == 0 && g == 0) a.tmp_s[prow] = Lsum > 0.f ? M + logf(Lsum) : -INFINITY;
#pragma unroll
  for (int i = 0; i < NDB / 4; ++i) {  // wave w finishes dim blocks [w NDB / 4, (w + 1) NDB / 4)
    const int db = wave * (NDB / 4) + i;
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) o += *(const f32x4 *)(ost + w * (L::STAGE / 4) + (db * 64 + lane) * 4) * wgt[w];
    o *= inv;
    const int d = 16 * db + 4 * g;
    if (part) *(f32x4 *)(a.tmp_v + prow * D + d) = o;
    else *(uint2 *)((T *)a.o + ((int64_t)b * a.H + head) * D + d) = make_uint2(Mma<T>::pk(o[0], o[1]), Mma<T>::pk(o[2], o[3]));
  }
}

// One workgroup per (request, head): o = v_scale sum_z e^(lse_z - M) O_z / sum_z e^(lse_z - M) over the request's plan tiles in index order; empty
// partials (lse = -inf) are not read.
template <class T>
__global__ void __launch_bounds__(64) merge_kernel(const float *tmp_v, const float *tmp_s, const int *o_indptr, T *o, int H, int D, float v_scale) {
  const int b = blockIdx.x, h = blockIdx.y, d = threadIdx.x * 4;
  const int z0 = o_indptr[b], z1 = o_indptr[b + 1];
  float M = -INFINITY;
  for (int z = z0; z < z1; ++z) M = fmaxf(M, tmp_s[(int64_t)z * H + h]);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  float wsum = 0.f;
  for (int z = z0; z < z1; ++z) {
    const float lse = tmp_s[(int64_t)z * H + h];
    if (!(lse > -INFINITY)) continue;
    const float w = expf(lse - M);
    wsum += w;
    acc += *(const f32x4 *)(tmp_v + ((int64_t)z * H + h) * D + d) * w;
  }
  acc *= wsum > 0.f ? v_scale / wsum : 0.f;
  T *op = o + ((int64_t)b * H + h) * D + d;
#pragma unroll
  for (int j = 0; j < 4; ++j) op[j] = from_f<T>(acc[j]);
}

template <class T, bool F8, int D, bool CAP> static void launch_one(const Args &a, int padded, hipStream_t s) {
  if (Lds<D>::BYTES > 64 * 1024) lds_attr_once((const void *)decode_kernel<T, F8, D, CAP>, Lds<D>::BYTES);  // D = 256 only
  hipLaunchKernelGGL((decode_kernel<T, F8, D, CAP>), dim3(padded, a.Hkv), dim3(256), Lds<D>::BYTES, s, a);
}
template <class T, bool F8, int D> static void launch_cap(const Args &a, int padded, hipStream_t s) {
  if (a.cap > 0.f) launch_one<T, F8, D, true>(a, padded, s);
  else launch_one<T, F8, D, false>(a, padded, s);
}
template <class T, bool F8> static void launch_dim(const Args &a, int D, int padded, hipStream_t s) {
  if (D == 64) launch_cap<T, F8, 64>(a, padded, s);
  else if (D == 128) launch_cap<T, F8, 128>(a, padded, s);
  else launch_cap<T, F8, 256>(a, padded, s);
}
template <class T> static int launch(const Args &a, bool f8, int D, int batch, int padded, hipStream_t s) {
  if (f8) launch_dim<T, true>(a, D, padded, s);
  else launch_dim<T, false>(a, D, padded, s);
  if (a.tmp_v) hipLaunchKernelGGL((merge_kernel<T>), dim3(batch, a.H), dim3(D / 4), 0, s, a.tmp_v, a.tmp_s, a.o_indptr, (T *)a.o, a.H, D, a.v_scale);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "flashinfer_decode: launch failed: %s\n", hipGetErrorString(e));
    return 7;
  }
  return 0;
}

}  // namespace fid
}  // namespace mrs

extern "C" void reshape_and_cache_flashinfer(void *key, void *value, void *key_cache, void *value_cache, int64_t *slot_mapping, int32_t num_tokens,
                                             int32_t num_heads, int32_t head_size, int32_t block_size, int32_t key_stride, int32_t value_stride,
                                             float k_scale, float v_scale, uint32_t dtype, uint32_t cache_dtype, mrs_stream_t stream) {
  using namespace mrs;
  if (num_tokens <= 0 || dtype > 2 || (cache_dtype != dtype && cache_dtype != 3)) return;
  hipStream_t s = (hipStream_t)stream;
#define MRS_FI_RESHAPE(T, F8)                                                                                                                        \
  hipLaunchKernelGGL((fid::reshape_and_cache_kernel<T, F8>), dim3(num_tokens), dim3(256), 0, s, (const T *)key, (const T *)value, key_cache, value_cache, \
                     slot_mapping, num_heads, head_size, block_size, key_stride, value_stride, k_scale, v_scale)
  const bool f8 = cache_dtype == 3;
  if (dtype == 0) { if (f8) MRS_FI_RESHAPE(f16_t, true); else MRS_FI_RESHAPE(f16_t, false); }
  else if (dtype == 1) { if (f8) MRS_FI_RESHAPE(bf16_t, true); else MRS_FI_RESHAPE(bf16_t, false); }
  else { if (f8) MRS_FI_RESHAPE(float, true); else MRS_FI_RESHAPE(float, false); }
#undef MRS_FI_RESHAPE
  fid::check_launch("reshape_and_cache_flashinfer");
}

extern "C" void gather_kv_cache_flashinfer(void *key_cache, void *value_cache, void *k_out, void *v_out, const int32_t *block_table,
                                           const int32_t *cu_seq_lens, int32_t num_tokens, int32_t num_seqs, int32_t block_size,
                                           int32_t block_table_stride, int32_t num_kv_heads, int32_t head_size, uint32_t out_dtype, uint32_t cache_dtype,
                                           float k_scale, float v_scale, mrs_stream_t stream) {
  using namespace mrs;
  if (num_tokens <= 0 || num_seqs <= 0 || out_dtype > 2 || (cache_dtype != out_dtype && cache_dtype != 3)) return;
  hipStream_t s = (hipStream_t)stream;
#define MRS_FI_GATHER(T, F8)                                                                                                                      \
  hipLaunchKernelGGL((fid::gather_kernel<T, F8>), dim3(num_tokens), dim3(256), 0, s, key_cache, value_cache, (T *)k_out, (T *)v_out, block_table, \
                     cu_seq_lens, num_seqs, block_size, block_table_stride, num_kv_heads, head_size, k_scale, v_scale)
  const bool f8 = cache_dtype == 3;
  if (out_dtype == 0) { if (f8) MRS_FI_GATHER(f16_t, true); else MRS_FI_GATHER(f16_t, false); }
  else if (out_dtype == 1) { if (f8) MRS_FI_GATHER(bf16_t, true); else MRS_FI_GATHER(bf16_t, false); }
  else { if (f8) MRS_FI_GATHER(float, true); else MRS_FI_GATHER(float, false); }
#undef MRS_FI_GATHER
  fid::check_launch("gather_kv_cache_flashinfer");
}

extern "C" int32_t flashinfer_decode(void *q, void *key_cache, void *value_cache, const int32_t *kv_indptr, const int32_t *kv_indices,
                                     const int32_t *kv_last_page_len, const int32_t *request_indices, const int32_t *kv_tile_indices,
                                     const int32_t *o_indptr, const int32_t *kv_chunk_size_ptr, const uint8_t *block_valid_mask, void *o, void *tmp_v,
                                     void *tmp_s, int32_t batch_size, int32_t padded_batch_size, int32_t num_qo_heads, int32_t num_kv_heads,
                                     int32_t head_size, int32_t page_size, int32_t q_stride_n, int32_t q_stride_h, float sm_scale, int32_t window_left,
                                     float logits_soft_cap, float k_scale, float v_scale, uint32_t dtype, uint32_t cache_dtype, mrs_stream_t stream) {
  using namespace mrs;
  if (dtype > 1) return 1;  // f16 / bf16 queries only
  if (cache_dtype != dtype && cache_dtype != 3) return 2;
  if (head_size != 64 && head_size != 128 && head_size != 256) return 3;
  if (page_size != 16 && page_size != 32) return 4;
  if (num_kv_heads < 1 || num_qo_heads < 1 || num_qo_heads % num_kv_heads || num_qo_heads / num_kv_heads > 16) return 5;
  if (padded_batch_size < batch_size || (tmp_v && !tmp_s) || (((uintptr_t)tmp_v | (uintptr_t)key_cache | (uintptr_t)value_cache | (uintptr_t)o) & 15)) return 6;
  if (batch_size <= 0) return 0;
  const fid::Args a{(const uint16_t *)q, key_cache, value_cache, kv_indptr, kv_indices, kv_last_page_len, request_indices, kv_tile_indices, o_indptr,
                    kv_chunk_size_ptr, block_valid_mask, o, (float *)tmp_v, (float *)tmp_s, sm_scale * k_scale, v_scale,
                    logits_soft_cap > 0.f ? logits_soft_cap : 0.f, num_qo_heads, num_kv_heads, num_qo_heads / num_kv_heads, page_size == 32 ? 5 : 4,
                    window_left, q_stride_n, q_stride_h};
  return dtype == 0 ? fid::launch<f16_t>(a, cache_dtype == 3, head_size, batch_size, padded_batch_size, (hipStream_t)stream)
                    : fid::launch<bf16_t>(a, cache_dtype == 3, head_size, batch_size, padded_batch_size, (hipStream_t)stream);
}
