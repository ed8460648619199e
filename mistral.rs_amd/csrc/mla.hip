// mla.hip -- multi-head latent attention (DeepSeek-V2 / V3) on the paged latent cache: the two cache ops and the decode kernel, gfx950 matrix cores.
//
// Role in the reference: `concat_and_cache_mla`, `gather_mla_cache` and `flashinfer_mla_decode` of mistralrs-paged-attn/src/cuda/ffi.rs:118-157,231-246
// (callers mistralrs-core/src/mla/forward.rs).  Semantics:
//   ckv_cache [num_blocks, block_size, 512]   kpe_cache [num_blocks, block_size, 64]   q_nope [batch, heads, 512]   q_pe [batch, heads, 64]
//   len_b = (indptr[b + 1] - indptr[b] - 1) * page_size + last_page_len[b] (0 without a page); key t lives in page indices[indptr[b] + t / page_size]
//   s[h, t] = sm_scale * (q_nope[b, h] . ckv[t] + q_pe[b, h] . kpe[t]);   out[b, h] = softmax_t(s[h]) . ckv   (zeros when len_b == 0)
//
// MI355X design.  The 512 latent values of a token are its key AND its value, and every head of a request reads the same row, so decode is a matrix
// product with M = heads.  One workgroup of four waves serves one request, one KV split and one block of 64 heads (32 when the model has no more).
// Wave w owns latent columns [128 w, 128 w + 128) and rotary dims [16 w, 16 w + 16): 144 of the 576 score dims, 9 MFMA k-steps, and the 128 output
// columns it alone accumulates.  Per 32-key tile:
//   * each wave copies ITS column slice of the tile from the pages into registers with 16-byte loads -- the NEXT tile's loads (and the page ids of
//     the tile after that) are issued before the current tile's MFMAs -- and from there into its own LDS region, twice: row-major with a 16-byte row
//     pad (the A fragment of S^T = C Q^T: lane = key, 8 consecutive dims, one ds_read_b128) and transposed, [column][key] with two keys per 32-bit
//     word and rows of 18 words (the B fragment of O += P C: lane = column, 2 x 4 consecutive keys, two ds_read_b64), the layout flash_attn_sinks.hip
//     uses for V.  No wave reads another wave's region, so staging needs no workgroup barrier, and a latent row leaves memory once per workgroup;
//   * the wave's partial S^T (32 keys x 64 heads over its 144 dims) goes to LDS as f32; after the tile's ONE workgroup barrier every wave adds the four
//     partials in wave order, so all four hold the same scores bit for bit.  The score buffer is double: a wave overwrites a buffer only two
//     barriers later.  Q is the B operand (its fragments stay in registers, 2 x 9), so a lane holds 16 keys of ONE head per head tile and the online
//     softmax is register math plus one exchange with lane ^ 32; P, rounded once to the tensor dtype, is in place the A fragment of O += P C;
//   * rows of keys >= the split's end are zeros written into LDS, never read from memory, and their scores are masked.
// Long contexts split over blockIdx.z: a split takes ceil(tiles / splits) tiles from the device-side length, writes its un-normalised f32 output and
// (max, sum) to the workspace (an empty one max = -inf, sum = 0), and a second launch merges the splits in order.  One split writes the output itself.
#include "common.cuh"
#include "mistralrs_paged_attn.h"
#include <float.h>
#include <math.h>
#include <stdio.h>

namespace mrs {
namespace mla {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

template <class T> struct Mma;
template <> struct Mma<bf16_t> {
  static __device__ __forceinline__ f32x16 run(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ unsigned pk(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  }
};
template <> struct Mma<f16_t> {
  static __device__ __forceinline__ f32x16 run(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ unsigned pk(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
  }
};

// ---------------------------------------------------------------------------------- cache ops
// One workgroup copies one token's latent row and rotary row.  16-byte accesses when both ends of a row are 16-byte aligned (every row is, once the
// base pointers and the row strides are), elements for the rest of the row or for all of it.
template <class E> __device__ __forceinline__ void copy_row(E *dst, const E *src, int n) {
  constexpr int EPC = 16 / (int)sizeof(E);
  int nv = 0;
  if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
    nv = n / EPC;
    for (int i = threadIdx.x; i < nv; i += blockDim.x) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
  }
  for (int i = nv * EPC + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

template <class E>
__global__ void __launch_bounds__(128) concat_and_cache_mla_kernel(const E *ckv, const E *k_pe, E *ckv_cache, E *kpe_cache, const int64_t *slot_mapping,
                                                                   int rank, int pe_dim, int ckv_stride, int kpe_stride) {
  const int64_t tok = blockIdx.x, slot = slot_mapping[tok];
  if (slot < 0) return;  // padding token
  copy_row(ckv_cache + slot * rank, ckv + tok * ckv_stride, rank);
  copy_row(kpe_cache + slot * pe_dim, k_pe + tok * kpe_stride, pe_dim);
}

template <class E>
__global__ void __launch_bounds__(128) gather_mla_cache_kernel(const E *ckv_cache, const E *kpe_cache, E *ckv_out, E *kpe_out, const int *block_table,
                                                               const int *cu_seq_lens, const int *token_to_seq, int block_size, int block_table_stride,
                                                               int rank, int pe_dim) {
  const int64_t tok = blockIdx.x;
  const int seq = token_to_seq[tok], pos = (int)tok - cu_seq_lens[seq];
  const int64_t row = (int64_t)block_table[(int64_t)seq * block_table_stride + pos / block_size] * block_size + pos % block_size;
  copy_row(ckv_out + tok * rank, ckv_cache + row * rank, rank);
  copy_row(kpe_out + tok * pe_dim, kpe_cache + row * pe_dim, pe_dim);
}

static void check_launch(const char *what) {  // a launch error ends the process, like the reference's CUDA_CHECK
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "%s: launch failed: %s\n", what, hipGetErrorString(e));
    abort();
  }
}

// ---------------------------------------------------------------------------------- decode
struct Args {
  const uint16_t *q_nope, *q_pe, *ckv, *kpe;
  const int *indptr, *indices, *last;
  void *out;
  float *ws_o, *ws_m, *ws_l;  // [batch, splits, heads, 512], [batch, splits, heads] x 2; unused with one split
  float scale;
  int heads, page_shift, splits;
};

constexpr int KT = 32;                   // keys per tile
constexpr int DC = 512, DR = 64;         // latent and rotary dims
constexpr int WC = DC / 4, WR = DR / 4;  // a wave's share of each
constexpr int K_ROW = (WC + WR) * 2 + 16;  // bytes of a row-major key row: 128 latent, 16 rotary, 16 bytes pad (19 chunks: odd, conflict-free b128 reads)
constexpr int K_BYTES = KT * K_ROW;
constexpr int V_ROW = 18;                // words of a transposed column: 16 key pairs + 2 pad
constexpr int V_BYTES = WC * V_ROW * 4;
constexpr int STAGE = K_BYTES + V_BYTES;  // per wave
template <int NR> struct Lds {
  static constexpr int SC_WAVE = NR * 1024;        // floats: [NR][4][64 lanes][4]
  static constexpr int SC_OFF = 4 * STAGE;         // two buffers of four waves
  static constexpr int BC_OFF = SC_OFF + 2 * 4 * SC_WAVE * 4;
  static constexpr int BYTES = BC_OFF + 4 * NR * 32 * 4;
};
static_assert(Lds<2>::BYTES <= LDS_DYN_MAX, "the 64-head kernel must fit the CU's LDS");

template <class T, int NR>
__global__ void __launch_bounds__(256) mla_decode_kernel(const Args a) {
  using L = Lds<NR>;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ql = lane & 31, kh = lane >> 5;
  const int b = blockIdx.x, h0 = blockIdx.y * 32 * NR, z = blockIdx.z;
  uint8_t *kst = smem + wave * STAGE;      // this wave's row-major slice
  unsigned *vst = (unsigned *)(kst + K_BYTES);   // this wave's transposed latent slice
  float *sc = (float *)(smem + L::SC_OFF);
  float *bc = (float *)(smem + L::BC_OFF) + wave * NR * 32;  // per-wave broadcast of per-head factors

  const int ip0 = a.indptr[b], npages = a.indptr[b + 1] - ip0;
  const int len = npages > 0 ? ((npages - 1) << a.page_shift) + a.last[b] : 0;
  const int ntile = (len + KT - 1) / KT, tps = (ntile + a.splits - 1) / a.splits;
  const int kbeg = min(z * tps, ntile) * KT, kend = min(len, (z + 1) * tps * KT);
  const int pmask = (1 << a.page_shift) - 1;

  // ---- Q fragments (B operand: lane = head ql, dims 16 ks + 8 kh .. + 8 of the wave's slice), resident for the whole key loop
  uint4 qf[NR][9];
#pragma unroll
  for (int rt = 0; rt < NR; ++rt) {
    const int head = h0 + rt * 32 + ql;
    const bool ok = head < a.heads;  // rows past the last head are zeros and are never stored
    const size_t row = (size_t)b * a.heads + (ok ? head : 0);
    const uint16_t *qn = a.q_nope + row * DC + WC * wave + 8 * kh;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[rt][ks] = ok ? *(const uint4 *)(qn + 16 * ks) : make_uint4(0, 0, 0, 0);
    qf[rt][8] = ok ? *(const uint4 *)(a.q_pe + row * DR + WR * wave + 8 * kh) : make_uint4(0, 0, 0, 0);
  }
  f32x16 o[NR][4];
#pragma unroll
  for (int rt = 0; rt < NR; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[rt][ct][r] = 0.f;
  float m[NR], l[NR];
#pragma unroll
  for (int rt = 0; rt < NR; ++rt) m[rt] = -FLT_MAX, l[rt] = 0.f;

  // ---- staging: pages -> registers -> this wave's LDS.  Latent: lane = (key pair p, chunk 4 i + c4), both keys of a pair share a page (sizes are even).
  const int p = lane >> 2, c4 = lane & 3;
  const int rk = lane >> 1, rc = lane & 1;  // rotary: lane = (key rk, chunk rc)
  uint4 creg[8], rreg;
  int pgc = 0, pgr = 0;  // page ids of the NEXT load
  auto pages = [&](int t0) {
    pgc = t0 + 2 * p < kend ? a.indices[ip0 + ((t0 + 2 * p) >> a.page_shift)] : 0;
    pgr = t0 + rk < kend ? a.indices[ip0 + ((t0 + rk) >> a.page_shift)] : 0;
  };
  auto load = [&](int t0) {
    const int k0 = t0 + 2 * p, k1 = t0 + rk;
    const uint16_t *cp = a.ckv + (((size_t)pgc << a.page_shift) + (k0 & pmask)) * DC + WC * wave + 8 * c4;
    const uint16_t *rp = a.kpe + (((size_t)pgr << a.page_shift) + (k1 & pmask)) * DR + WR * wave + 8 * rc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      creg[2 * i] = k0 < kend ? *(const uint4 *)(cp + 32 * i) : make_uint4(0, 0, 0, 0);
      creg[2 * i + 1] = k0 + 1 < kend ? *(const uint4 *)(cp + DC + 32 * i) : make_uint4(0, 0, 0, 0);
    }
    rreg = k1 < kend ? *(const uint4 *)rp : make_uint4(0, 0, 0, 0);
    pages(t0 + KT);
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 4 * i + c4;
      *(uint4 *)(kst + (2 * p) * K_ROW + c * 16) = creg[2 * i];
      *(uint4 *)(kst + (2 * p + 1) * K_ROW + c * 16) = creg[2 * i + 1];
      unsigned *vt = vst + (c * 8) * V_ROW + p;  // transposed: word [column][p] = (C[2p][column], C[2p + 1][column])
      const unsigned e[4] = {creg[2 * i].x, creg[2 * i].y, creg[2 * i].z, creg[2 * i].w};
      const unsigned f[4] = {creg[2 * i + 1].x, creg[2 * i + 1].y, creg[2 * i + 1].z, creg[2 * i + 1].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vt[(2 * j) * V_ROW] = (e[j] & 0xffffu) | (f[j] << 16);
        vt[(2 * j + 1) * V_ROW] = (e[j] >> 16) | (f[j] & 0xffff0000u);
      }
    }
    *(uint4 *)(kst + rk * K_ROW + WC * 2 + rc * 16) = rreg;
  };

  if (kbeg < kend) {
    pages(kbeg);
    load(kbeg);
  }
  int buf = 0;
  for (int t0 = kbeg; t0 < kend; t0 += KT, buf ^= 1) {
    MRS_WAVE_SYNC();  // the wave's reads of the previous tile are issued before its region is overwritten
    store();
    MRS_WAVE_SYNC();
    if (t0 + KT < kend) load(t0 + KT);
    // ---- this wave's share of S^T = C Q^T (32 keys x 32 heads per head tile) over its 144 dims
    f32x16 sacc[NR];
#pragma unroll
    for (int rt = 0; rt < NR; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[rt][r] = 0.f;
    {
      const uint8_t *kp = kst + ql * K_ROW + kh * 16;
#pragma unroll
      for (int ks = 0; ks < 9; ++ks) {
        const uint4 af = *(const uint4 *)(kp + ks * 32);
#pragma unroll
        for (int rt = 0; rt < NR; ++rt) sacc[rt] = Mma<T>::run(af, qf[rt][ks], sacc[rt]);
      }
    }
    float *sb = sc + buf * (4 * L::SC_WAVE);
#pragma unroll
    for (int rt = 0; rt < NR; ++rt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *(float4 *)(sb + wave * L::SC_WAVE + ((rt * 4 + g4) * 64 + lane) * 4) =
            make_float4(sacc[rt][4 * g4], sacc[rt][4 * g4 + 1], sacc[rt][4 * g4 + 2], sacc[rt][4 * g4 + 3]);
    __syncthreads();  // the tile's only workgroup barrier
#pragma unroll
    for (int rt = 0; rt < NR; ++rt) {
      // ---- the four partials in wave order, then the online softmax of head ql: this lane holds keys (r & 3) + 8 (r >> 2) + 4 kh of the tile
      float sv[16], mx = -FLT_MAX;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float *sp = sb + ((rt * 4 + g4) * 64 + lane) * 4;
        float4 s4 = *(const float4 *)sp;
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const float4 t4 = *(const float4 *)(sp + w * L::SC_WAVE);
          s4.x += t4.x; s4.y += t4.y; s4.z += t4.z; s4.w += t4.w;
        }
        sv[4 * g4] = s4.x; sv[4 * g4 + 1] = s4.y; sv[4 * g4 + 2] = s4.z; sv[4 * g4 + 3] = s4.w;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kpos = t0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        sv[r] = kpos < kend ? sv[r] * a.scale : -FLT_MAX;
        mx = fmaxf(mx, sv[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m[rt], mx);
      const float alpha = __expf(m[rt] - mn);
      float pr[16], ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pr[r] = sv[r] > -FLT_MAX ? __expf(sv[r] - mn) : 0.f;
        ps += pr[r];
      }
      ps += __shfl_xor(ps, 32, 64);
      l[rt] = l[rt] * alpha + ps;
      m[rt] = mn;
      // ---- rescale O: accumulator register r of a lane belongs to head row (r & 3) + 8 (r >> 2) + 4 kh
      if (kh == 0) bc[rt * 32 + ql] = alpha;
      MRS_WAVE_SYNC();
      float ar[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 t4 = *(const float4 *)(bc + rt * 32 + 8 * g4 + 4 * kh);
        ar[4 * g4] = t4.x; ar[4 * g4 + 1] = t4.y; ar[4 * g4 + 2] = t4.z; ar[4 * g4 + 3] = t4.w;
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[rt][ct][r] *= ar[r];
      // ---- O += P C on the wave's 128 columns: P is the score registers in place, rounded once to the tensor dtype
      const unsigned *vp = vst + ql * V_ROW + 2 * kh;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint4 pf = make_uint4(Mma<T>::pk(pr[8 * s], pr[8 * s + 1]), Mma<T>::pk(pr[8 * s + 2], pr[8 * s + 3]),
                                    Mma<T>::pk(pr[8 * s + 4], pr[8 * s + 5]), Mma<T>::pk(pr[8 * s + 6], pr[8 * s + 7]));
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const uint2 v0 = *(const uint2 *)(vp + ct * 32 * V_ROW + 8 * s), v1 = *(const uint2 *)(vp + ct * 32 * V_ROW + 8 * s + 4);
          o[rt][ct] = Mma<T>::run(pf, make_uint4(v0.x, v0.y, v1.x, v1.y), o[rt][ct]);
        }
      }
    }
  }

  // ---- one split: normalise and store.  More: the un-normalised f32 columns and (max, sum) for the merge
  const bool direct = a.splits == 1;
#pragma unroll
  for (int rt = 0; rt < NR; ++rt) {
    MRS_WAVE_SYNC();
    if (kh == 0) bc[rt * 32 + ql] = direct ? (l[rt] > 0.f ? 1.f / l[rt] : 0.f) : 1.f;
    MRS_WAVE_SYNC();
    float inv[16];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const float4 t4 = *(const float4 *)(bc + rt * 32 + 8 * g4 + 4 * kh);
      inv[4 * g4] = t4.x; inv[4 * g4 + 1] = t4.y; inv[4 * g4 + 2] = t4.z; inv[4 * g4 + 3] = t4.w;
    }
    const size_t prow = ((size_t)b * a.splits + z) * a.heads;  // this split's first workspace row
    if (!direct && wave == 0 && kh == 0 && h0 + rt * 32 + ql < a.heads) {
      a.ws_m[prow + h0 + rt * 32 + ql] = l[rt] > 0.f ? m[rt] : -INFINITY;
      a.ws_l[prow + h0 + rt * 32 + ql] = l[rt];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int head = h0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (head >= a.heads) continue;
      const int col = WC * wave + ql;
      if (direct) {
        T *op = (T *)a.out + ((size_t)b * a.heads + head) * DC + col;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) op[ct * 32] = from_f<T>(o[rt][ct][r] * inv[r]);
      } else {
        float *op = a.ws_o + (prow + head) * DC + col;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) op[ct * 32] = o[rt][ct][r];
      }
    }
  }
}

// One workgroup per (request, head): out = sum_z e^(m_z - M) O_z / sum_z e^(m_z - M) l_z, splits taken in order; empty splits (l == 0) are not read.
template <class T>
__global__ void __launch_bounds__(128) mla_merge_kernel(const float *ws_o, const float *ws_m, const float *ws_l, T *out, int heads, int splits) {
  const int b = blockIdx.x, h = blockIdx.y, d = threadIdx.x * 4;
  float M = -INFINITY;
  for (int z = 0; z < splits; ++z) M = fmaxf(M, ws_m[((size_t)b * splits + z) * heads + h]);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float lsum = 0.f;
  for (int z = 0; z < splits; ++z) {
    const size_t row = ((size_t)b * splits + z) * heads + h;
    const float lz = ws_l[row];
    if (!(lz > 0.f)) continue;
    const float w = expf(ws_m[row] - M);
    const float4 v = *(const float4 *)(ws_o + row * DC + d);
    lsum += w * lz;
    acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
  }
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
  T *op = out + ((size_t)b * heads + h) * DC + d;
  op[0] = from_f<T>(acc.x * inv); op[1] = from_f<T>(acc.y * inv); op[2] = from_f<T>(acc.z * inv); op[3] = from_f<T>(acc.w * inv);
}

static size_t workspace_bytes(int batch, int heads, int splits) {
  return splits > 1 && batch > 0 && heads > 0 ? (size_t)batch * splits * heads * (DC + 2) * sizeof(float) : 0;
}

template <class T> static int launch(Args a, int batch, hipStream_t s) {
  const dim3 grid(batch, a.heads > 32 ? (a.heads + 63) / 64 : 1, a.splits);
  if (a.heads > 32) {
    lds_attr_once((const void *)mla_decode_kernel<T, 2>, Lds<2>::BYTES);
    hipLaunchKernelGGL((mla_decode_kernel<T, 2>), grid, dim3(256), Lds<2>::BYTES, s, a);
  } else {
    lds_attr_once((const void *)mla_decode_kernel<T, 1>, Lds<1>::BYTES);
    hipLaunchKernelGGL((mla_decode_kernel<T, 1>), grid, dim3(256), Lds<1>::BYTES, s, a);
  }
  if (a.splits > 1)
    hipLaunchKernelGGL((mla_merge_kernel<T>), dim3(batch, a.heads), dim3(128), 0, s, a.ws_o, a.ws_m, a.ws_l, (T *)a.out, a.heads, a.splits);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "launch_mla_decode: launch failed: %s\n", hipGetErrorString(e));
    return 5;
  }
  return 0;
}

}  // namespace mla
}  // namespace mrs

extern "C" void concat_and_cache_mla(const void *ckv, const void *k_pe, void *ckv_cache, void *kpe_cache, const int64_t *slot_mapping,
                                     int num_tokens, int kv_lora_rank, int kpe_head_dim, int block_size, int ckv_stride, int kpe_stride,
                                     void *stream, uint32_t dtype) {
  (void)block_size;  // a slot is block * block_size + row, and the caches are contiguous
  if (num_tokens <= 0 || dtype > 2) return;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 2)
    hipLaunchKernelGGL((mrs::mla::concat_and_cache_mla_kernel<uint32_t>), dim3(num_tokens), dim3(128), 0, s, (const uint32_t *)ckv, (const uint32_t *)k_pe,
                       (uint32_t *)ckv_cache, (uint32_t *)kpe_cache, slot_mapping, kv_lora_rank, kpe_head_dim, ckv_stride, kpe_stride);
  else
    hipLaunchKernelGGL((mrs::mla::concat_and_cache_mla_kernel<uint16_t>), dim3(num_tokens), dim3(128), 0, s, (const uint16_t *)ckv, (const uint16_t *)k_pe,
                       (uint16_t *)ckv_cache, (uint16_t *)kpe_cache, slot_mapping, kv_lora_rank, kpe_head_dim, ckv_stride, kpe_stride);
  mrs::mla::check_launch("concat_and_cache_mla");
}

extern "C" void gather_mla_cache(const void *ckv_cache, const void *kpe_cache, void *ckv_out, void *kpe_out, const int *block_table,
                                 const int *cu_seq_lens, const int *token_to_seq, int num_tokens, int block_size, int block_table_stride,
                                 int kv_lora_rank, int kpe_head_dim, void *stream, uint32_t dtype) {
  if (num_tokens <= 0 || dtype > 2) return;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 2)
    hipLaunchKernelGGL((mrs::mla::gather_mla_cache_kernel<uint32_t>), dim3(num_tokens), dim3(128), 0, s, (const uint32_t *)ckv_cache,
                       (const uint32_t *)kpe_cache, (uint32_t *)ckv_out, (uint32_t *)kpe_out, block_table, cu_seq_lens, token_to_seq, block_size,
                       block_table_stride, kv_lora_rank, kpe_head_dim);
  else
    hipLaunchKernelGGL((mrs::mla::gather_mla_cache_kernel<uint16_t>), dim3(num_tokens), dim3(128), 0, s, (const uint16_t *)ckv_cache,
                       (const uint16_t *)kpe_cache, (uint16_t *)ckv_out, (uint16_t *)kpe_out, block_table, cu_seq_lens, token_to_seq, block_size,
                       block_table_stride, kv_lora_rank, kpe_head_dim);
  mrs::mla::check_launch("gather_mla_cache");
}

extern "C" size_t mla_decode_workspace_bytes(int batch_size, int num_qo_heads, int num_splits) {
  return mrs::mla::workspace_bytes(batch_size, num_qo_heads, num_splits);
}

extern "C" int launch_mla_decode(const void *q_nope, const void *q_pe, const void *ckv_cache, const void *kpe_cache, const int *kv_indptr,
                                 const int *kv_indices, const int *kv_last_page_len, void *out, int batch_size, int num_qo_heads, int page_size,
                                 float sm_scale, int num_splits, void *workspace, size_t workspace_bytes, uint32_t dtype, void *stream) {
  if (dtype > 1) return 1;  // f16 / bf16 only: nobody keeps an f32 latent cache
  if (page_size != 16 && page_size != 32) return 2;
  if (num_qo_heads < 1 || num_splits < 1 || num_splits > 65535) return 3;
  if (batch_size <= 0) return 0;
  const size_t need = mrs::mla::workspace_bytes(batch_size, num_qo_heads, num_splits);
  if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))) return 4;
  float *ws = (float *)workspace;
  const size_t rows = (size_t)batch_size * num_splits * num_qo_heads;
  const mrs::mla::Args a{(const uint16_t *)q_nope, (const uint16_t *)q_pe, (const uint16_t *)ckv_cache, (const uint16_t *)kpe_cache,
                         kv_indptr, kv_indices, kv_last_page_len, out, ws, need ? ws + rows * mrs::mla::DC : nullptr,
                         need ? ws + rows * (mrs::mla::DC + 1) : nullptr, sm_scale, num_qo_heads, page_size == 32 ? 5 : 4, num_splits};
  return dtype == 0 ? mrs::mla::launch<mrs::f16_t>(a, batch_size, (hipStream_t)stream)
                    : mrs::mla::launch<mrs::bf16_t>(a, batch_size, (hipStream_t)stream);
}

extern "C" int flashinfer_mla_decode(const void *q_nope, const void *q_pe, const void *ckv_cache, const void *kpe_cache, const int *kv_indptr,
                                     const int *kv_indices, const int *kv_last_page_len, void *out, int batch_size, int num_qo_heads, int page_size,
                                     float sm_scale, int window_left, float logits_soft_cap, float rope_scale, float rope_theta,
                                     const int *request_indices, const int *kv_tile_indices, const int *o_indptr, const int *kv_chunk_size_ptr,
                                     uint32_t dtype, void *stream) {
  // Q and K arrive rotated (the reference passes rope_scale = rope_theta = 1) and the split is chosen by the caller of launch_mla_decode, not by a
  // tile plan: the four plan pointers are not read
  (void)rope_scale; (void)rope_theta; (void)request_indices; (void)kv_tile_indices; (void)o_indptr; (void)kv_chunk_size_ptr;
  if (window_left >= 0 || logits_soft_cap != 0.f) return 6;
  return launch_mla_decode(q_nope, q_pe, ckv_cache, kpe_cache, kv_indptr, kv_indices, kv_last_page_len, out, batch_size, num_qo_heads, page_size,
                           sm_scale, 1, nullptr, 0, dtype, stream);
}
