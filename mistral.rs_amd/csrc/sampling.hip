// sampling.hip -- libmistralrscuda, sampling subset.  A MAP of this file: three two-stage families over rows of 100k+ f32 logits, the helpers they share, and the
// arithmetic each helper pins.  (Further down, apart from all this: the sparse penalties / bias pre-processing,
// one row at a time as the reference exports it, and mrs_penalties_f32_batched, every row of a step in one launch from the raw token history.)  The caller owns every buffer.
//
// The families -- stage 1 is one workgroup of NT threads per `chunk_size` logits, stage 2 one workgroup per row; the row is always a block index:
//   top-k        topk_large_f32, topk_large_f32_packed, topk_large_f32_packed_batched      mistralrs-core/src/cuda/sort.cu:1502-1823,2146-2206 ; ffi.rs:583-624 ;
//                caller ops.rs:691-828 (cuda_topk_logits_f32_packed); top-p / min-p / the multinomial draw stay on the host (Sampler::sample_topk_on_device,
//                mistralrs-core/src/sampler.rs:1171-1260).
//                stage 1: block_values / block_indices [chunk][k] = the chunk's k largest logits in (value descending, index ascending) order, NaN and -inf never
//                selected, missing entries (-inf, 0); block_maxes[chunk] = top value * inv_temperature (-inf for an empty chunk); block_sums[chunk] = the chunk's
//                share of the normaliser.  stage 2: global max of block_maxes, denom = sum_b block_sums[b] * expf(block_maxes[b] - max), the k best candidates in
//                the same order; packed_out = [k values][k indices as f32][denom][max].
//   greedy       top1_large_f32_packed, top1_large_f32_packed_batched                      sort.cu:1825-1912,2071-2143,2207-2238 ; ffi.rs:643-665 ; caller ops.rs:1232-2000.
//                No softmax: block_argmax twice.  Shares only the candidate key with the others.
//   draws        categorical_large_f32_packed_batched (sort.cu:1825-2069,2240-2257 ; ffi.rs:666 ; caller ops.rs:1347-1500: temperature only) and
//                mrs_nucleus_large_f32_packed_batched (top-p / min-p over the whole row; no reference counterpart).  ONE stage 1, cat_stage1_kernel: block_values =
//                the chunk's largest raw logit (NaN if it holds one), block_sums = the chunk's share under block_value * inv_t.  Two stage 2s behind one row preamble:
//                cat_stage2_kernel inverts f32 running sums, nuc_stage2_kernel fixed-point integer masses -- they may draw different tokens and stay apart.
//
// The shared helpers, and what each one pins:
//   order_key / order_key_value    the float <-> order-preserving unsigned mapping (-0.0 == +0.0).  key_of / val_of / idx_of build the 64-bit candidate key of
//                                  top-k and greedy on it; the nucleus radix select reads its digits from it.
//   load_chunk                     the chunk in registers, thread-strided (local = tid + NT j).  Both stage 1s; the partial sums below depend on this assignment.
//   chunk_softmax_share            block_sums: sum of expf(x * inv_t - block_max), NaN rule included, in the reference's association (per-thread strided partials,
//                                  block_sum_ref_order: 32-lane shuffle-down trees, warp sums through LDS), so that only expf's last ulp separates the normaliser
//                                  from the CUDA build's.  Both stage 1s: the three entry points leave bit-identical block_sums for the same logits and temperature.
//   block_max_nan<WAVES>           workgroup max with a carried NaN flag: cat_stage1_kernel (4 waves) and, through the preamble, both draw stage 2s (4 and 16 waves).
//   row_preamble<NTH>, chunk_mass  gmax, the chunk masses, denom = their sum by ONE thread in ascending chunk index, the validity expression.  Both draw stage 2s:
//                                  the logprob of either draw is x * inv_t - gmax - logf(denom) with this gmax and this denom.
//   store_nan_row                  the unusable-row report of both draws.      draw_shape_ok: the launch refusals of both draws.
//   head_merge, wave_max_u64       top-k only (stage 1's merge of four wave lists, stage 2's merge of nblocks lists).      block_argmax: greedy only.
//
// MI355X design of top-k (not the reference's k rounds of scan-the-chunk + two block barriers each):
//   stage 1: every wave extracts the top-k of its quarter of the register-resident chunk on its own -- one 64-bit key per candidate (order key << 32 | ~index, so ONE
//   max reduction per round settles value and tie; DPP + v_readlane, no LDS crossbar), each lane's keys sorted once so that its best is keys[0], no barrier -- then
//   wave 0 merges the four sorted lists by heads (one lane per list).  stage 2 is the same head merge over the nblocks sorted lists (a lane per list, lists beyond 64
//   share lanes): k rounds of one wave-wide max instead of k scans of nblocks * k candidates.
#include "common.cuh"
#include <stdint.h>
#include <algorithm>

namespace mrs {
namespace sampling {

constexpr int NT = 256;       // threads per workgroup (the reference's block size: the strided partial sums depend on it)
constexpr int MAXV = 16;      // logits per thread kept in registers: chunks up to 4096
constexpr int MAX_K = 128;    // CUDA_TOPK_MAX_K (ops.rs:18)

// One 64-bit key per candidate: [63:32] the value's bits mapped to an order-preserving unsigned (with -0.0 == +0.0, as the reference's `>` sees them),
// [31:1] ~index (so the LOWER index wins a tie; indices < 2^31), [0] "the value was -0.0" (to give back the original bits).  0 = not a candidate.
__device__ __forceinline__ unsigned order_key(float v) {  // a > b <=> order_key(a) > order_key(b), with -0.0 == +0.0; NaN never gets here
  const unsigned u = __float_as_uint(v + 0.0f);   // -0.0 -> +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_key_value(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
__device__ __forceinline__ unsigned long long key_of(float v, unsigned idx) {
  // NaN and -inf are never candidates (sort.cu:1552: candidate == candidate && candidate > -INFINITY)
  if (!(v == v) || v == -INFINITY) return 0ull;
  const unsigned o = order_key(v);
  const unsigned low = ((~idx) << 1) | (__float_as_uint(v) == 0x80000000u ? 1u : 0u);
  return ((unsigned long long)o << 32) | (unsigned long long)low;
}
__device__ __forceinline__ unsigned idx_of(unsigned long long key) { return (~((unsigned)key >> 1)) & 0x7fffffffu; }
__device__ __forceinline__ float val_of(unsigned long long key) {  // the candidate's original bits
  return ((unsigned)key & 1u) ? -0.0f : order_key_value((unsigned)(key >> 32));
}
// max over the wave, every lane gets it: DPP inside rows of 16 (xor 1, xor 2, half-row mirror, row mirror), then the four row results through v_readlane -- no LDS crossbar
template <int CTRL> __device__ __forceinline__ unsigned long long dpp_u64(unsigned long long k) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)k, CTRL, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(k >> 32), CTRL, 0xf, 0xf, false);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long k, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
  unsigned long long o;
  o = dpp_u64<0xB1>(k); k = o > k ? o : k;
  o = dpp_u64<0x4E>(k); k = o > k ? o : k;
  o = dpp_u64<0x141>(k); k = o > k ? o : k;
  o = dpp_u64<0x140>(k); k = o > k ? o : k;
  const unsigned long long r0 = readlane_u64(k, 0), r1 = readlane_u64(k, 16), r2 = readlane_u64(k, 32), r3 = readlane_u64(k, 48);
  const unsigned long long a = r0 > r1 ? r0 : r1, b = r2 > r3 ? r2 : r3;
  return a > b ? a : b;
}
// the reference's reductions, association for association (sort.cu:1470-1497): 32-lane shuffle-down trees, warp sums through shared memory, first warp again
__device__ __forceinline__ float warp32_sum_down(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_down(v, off, 32);
  return v;
}
__device__ __forceinline__ float block_sum_ref_order(float v, float *warp_sums /* [32] */) {
  const int tid = threadIdx.x, warp_id = tid / 32, lane_id = tid % 32;
  v = warp32_sum_down(v);
  if (lane_id == 0) warp_sums[warp_id] = v;
  __syncthreads();
  v = tid < NT / 32 ? warp_sums[tid] : 0.0f;
  if (tid < 64) v = warp32_sum_down(v);  // the whole first wave walks the tree (lanes 32..63 reduce zeros): lane 0 sees the reference's first-warp tree
  __syncthreads();
  return v;  // valid in thread 0
}

// ---- stage 1 shared by the three families.  A chunk of up to NT * MAXV logits lives in REGISTERS in the reference's thread-strided assignment (local = tid + NT j;
// -inf beyond `width`): the per-thread partial sums below depend on exactly this assignment.
__device__ __forceinline__ void load_chunk(const float *chunk, int width, float (&v)[MAXV]) {
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    const int local = threadIdx.x + j * NT;
    v[j] = local < width ? chunk[local] : -INFINITY;
  }
}
// the chunk's share of the softmax normaliser (sort.cu:1580-1597): sum of expf(x * inv_t - block_max), NaN if the chunk holds one, 0 when `empty` (nothing in the
// chunk is selectable: block_max is -inf).  Expression, NaN rule and association are the reference's: nothing here may be reordered.  Valid in thread 0; two barriers.
__device__ __forceinline__ float chunk_softmax_share(const float (&v)[MAXV], int width, float inv_t, float block_max, bool empty) {
  __shared__ float s_warp_sums[32];
  float local_sum = 0.0f;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    const int local = threadIdx.x + j * NT;
    if (local < width) {
      const float c = v[j];
      if (c != c) local_sum = NAN;
      else if (!empty) local_sum += expf(c * inv_t - block_max);
    }
  }
  return block_sum_ref_order(local_sum, s_warp_sums);
}
// workgroup max of the threads' `m` with a carried NaN flag (fmaxf drops a NaN, so a thread that met one passes nan = true and keeps it out of m): every thread gets
// the max of the rest and, in `any_nan`, the OR of the flags.  A max and an OR: the fold order is free.  One barrier.  The LDS slots are not recycled inside
// the call: a kernel that calls it again (spec_stage1_kernel, row_preamble in a loop) must put a barrier between one call's reads of the slots -- they end where the call
// returns -- and the next call's writes (chunk_softmax_share's two barriers, or a __syncthreads after the preamble, do that).
template <int WAVES> __device__ __forceinline__ float block_max_nan(float m, bool nan, bool &any_nan) {
  __shared__ float s_wmax[WAVES];
  __shared__ int s_wnan[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  m = wave_max(m);
  const bool wave_nan = __ballot(nan) != 0ull;
  if (lane == 0) { s_wmax[wave] = m; s_wnan[wave] = wave_nan ? 1 : 0; }
  __syncthreads();
  int nans = 0;
  float r = -INFINITY;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) { nans |= s_wnan[i]; r = fmaxf(r, s_wmax[i]); }
  any_nan = nans != 0;
  return r;
}

struct Stage1Args {
  const float *input;
  float *block_values;
  uint32_t *block_indices;
  float *block_maxes, *block_sums;
  const float *inv_temperatures;  // one per row, or NULL: every row takes the scalar
  float inv_temperature;
  int ncols, k, chunk_size, nblocks;
};

// merge `nl` lists sorted by key (descending) into the k best: lane l walks list l (l, l + 64, ... when nl > 64) by its head and keeps the best of its heads in a
// register; one wave-wide max per round, and only the WINNING lane does anything else (win(ki, list, pos), advance its head, refresh its best) -- no broadcast.
// `get(list, pos)` returns the key (0 = exhausted); without a winner lane 0 calls win(ki, -1, 0).  One wave.
template <class Get, class Win>
__device__ __forceinline__ void head_merge(int nl, int k, int *heads /* LDS [nl] */, Get get, Win win) {
  const int lane = threadIdx.x & 63;
  for (int l = lane; l < nl; l += 64) heads[l] = 0;  // a lane only ever touches the heads of its own lists: no cross-lane traffic through LDS
  int bl = -1;
  auto my_best = [&]() {
    unsigned long long b = 0ull;
    bl = -1;
    for (int l = lane; l < nl; l += 64) {
      const int h = heads[l];
      const unsigned long long key = h < k ? get(l, h) : 0ull;
      if (key > b) { b = key; bl = l; }
    }
    return b;
  };
  unsigned long long best = my_best();
  for (int ki = 0; ki < k; ++ki) {
    const unsigned long long w = wave_max_u64(best);
    if (w != 0ull && best == w) {  // keys are unique (they carry the index): exactly one lane
      const int pos = heads[bl];
      win(ki, bl, pos);
      heads[bl] = pos + 1;
      best = my_best();
    } else if (w == 0ull && lane == 0) {
      win(ki, -1, 0);
    }
  }
}

__global__ void __launch_bounds__(NT) topk_stage1_kernel(Stage1Args a) {
  __shared__ unsigned long long s_keys[4][MAX_K];  // each wave's sorted candidates
  __shared__ int s_heads[4];
  __shared__ float s_block_max;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row = blockIdx.y;
  const int chunk = blockIdx.x, k = a.k;
  const float *input = a.input + row * (size_t)a.ncols;
  float *bv = a.block_values + (row * a.nblocks + chunk) * (size_t)k;
  uint32_t *bi = a.block_indices + (row * a.nblocks + chunk) * (size_t)k;
  const float inv_t = a.inv_temperatures ? a.inv_temperatures[row] : a.inv_temperature;
  const int start = chunk * a.chunk_size, end = min(start + a.chunk_size, a.ncols), width = max(0, end - start);
  float v[MAXV];
  unsigned long long keys[MAXV];
  load_chunk(input + start, width, v);
#pragma unroll
  for (int j = 0; j < MAXV; ++j) keys[j] = key_of(v[j], (unsigned)(start + tid + j * NT));  // the -inf beyond the chunk is no candidate
  // ---- every wave: the k best of its 64 x MAXV logits, sorted.  Each lane first sorts ITS keys (descending, a bitonic network in registers), so that its
  // best unused key is always keys[0]; the round's winner shifts its array down by one.  A round = one wave-wide 64-bit max + 2 * MAXV moves in one lane.
#pragma unroll
  for (int size = 2; size <= MAXV; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1)
#pragma unroll
      for (int j = 0; j < MAXV; ++j) {
        const int p = j ^ stride;
        if (p > j) {
          const bool desc = (j & size) == 0;  // direction of this bitonic block
          const unsigned long long a = keys[j], b = keys[p];
          const bool sw = desc ? a < b : a > b;
          keys[j] = sw ? b : a;
          keys[p] = sw ? a : b;
        }
      }
  for (int ki = 0; ki < k; ++ki) {
    const unsigned long long win = wave_max_u64(keys[0]);
    if (win != 0ull && keys[0] == win) {  // keys carry the index: exactly one lane
      s_keys[wave][ki] = win;
#pragma unroll
      for (int j = 0; j + 1 < MAXV; ++j) keys[j] = keys[j + 1];
      keys[MAXV - 1] = 0ull;
    } else if (win == 0ull && lane == 0) {
      s_keys[wave][ki] = 0ull;
    }
  }
  __syncthreads();
  // ---- wave 0: merge the four lists
  if (wave == 0) {
    head_merge(4, k, s_heads, [&](int l, int h) { return s_keys[l][h]; },
               [&](int ki, int wl, int wp) {  // the winning lane (or lane 0 when nothing is left)
                 const unsigned long long key = wl >= 0 ? s_keys[wl][wp] : 0ull;
                 bv[ki] = wl >= 0 ? val_of(key) : -INFINITY;
                 bi[ki] = wl >= 0 ? idx_of(key) : 0u;
                 if (ki == 0) s_block_max = width > 0 ? (wl >= 0 ? val_of(key) : -INFINITY) * inv_t : -INFINITY;
               });
  }
  __syncthreads();
  const float block_max = s_block_max;
  const float block_sum = chunk_softmax_share(v, width, inv_t, block_max, block_max == -INFINITY);
  if (tid == 0) {
    a.block_maxes[row * a.nblocks + chunk] = block_max;
    a.block_sums[row * a.nblocks + chunk] = block_sum;
  }
}

struct Stage2Args {
  const float *block_values;
  const uint32_t *block_indices;
  const float *block_maxes, *block_sums;
  float *packed_out;      // [2k + 2] per row, or NULL
  float *values_out;      // unpacked variant
  uint32_t *indices_out;
  float *softmax_info_out;
  int nblocks, k, depth;
};

__global__ void __launch_bounds__(NT) topk_stage2_kernel(Stage2Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int *heads = (int *)smem;  // [nblocks]
  __shared__ float s_warp_max[32], s_warp_sums[32];
  __shared__ float s_global_max;
  const int tid = threadIdx.x, lane = tid & 63, k = a.k, nb = a.nblocks;
  const size_t row = blockIdx.x;
  const float *bv = a.block_values + row * (size_t)nb * k;
  const uint32_t *bi = a.block_indices + row * (size_t)nb * k;
  const float *bm = a.block_maxes + row * (size_t)nb, *bs = a.block_sums + row * (size_t)nb;
  float *packed = a.packed_out ? a.packed_out + row * (size_t)(2 * k + 2) : nullptr;
  // global max (a max is association-free)
  float gm = -INFINITY;
  for (int b = tid; b < nb; b += NT) gm = fmaxf(gm, bm[b]);
  gm = wave_max(gm);
  if (lane == 0) s_warp_max[tid >> 6] = gm;
  __syncthreads();
  if (tid == 0) s_global_max = fmaxf(fmaxf(s_warp_max[0], s_warp_max[1]), fmaxf(s_warp_max[2], s_warp_max[3]));
  __syncthreads();
  const float global_max = s_global_max;
  float local_denom = 0.0f;
  if (global_max != -INFINITY)
    for (int b = tid; b < nb; b += NT) local_denom += bs[b] * expf(bm[b] - global_max);
  const float denom = block_sum_ref_order(local_denom, s_warp_sums);
  if (tid == 0) {
    if (packed) { packed[2 * k] = denom; packed[2 * k + 1] = global_max; }
    else { a.softmax_info_out[0] = denom; a.softmax_info_out[1] = global_max; }
  }
  // the heads of every list, as keys, in LDS: `depth` entries per list (all k of them for vocabularies up to ~130k tokens); deeper entries are read from memory
  unsigned long long *skeys = (unsigned long long *)(smem + (((size_t)nb * sizeof(int) + 7) & ~(size_t)7));
  const int depth = a.depth;
  for (int i = tid; i < nb * depth; i += NT) {
    const int l = i / depth, h = i - l * depth;
    skeys[i] = key_of(bv[(size_t)l * k + h], bi[(size_t)l * k + h]);
  }
  __syncthreads();
  if (tid >= 64) return;
  // winners are only RECORDED in the loop (list, position); values and indices are gathered afterwards by 64 lanes at once -- a load per round on the
  // critical path would cost more than the round itself
  __shared__ int s_win[MAX_K];
  head_merge(nb, k, heads, [&](int l, int h) { return h < depth ? skeys[l * depth + h] : key_of(bv[(size_t)l * k + h], bi[(size_t)l * k + h]); },
             [&](int ki, int wl, int wp) { s_win[ki] = wl >= 0 ? wl * k + wp : -1; });
  MRS_WAVE_SYNC();
  for (int ki = lane; ki < k; ki += 64) {
    const int pos = s_win[ki];
    const float val = pos >= 0 ? bv[pos] : -INFINITY;
    const uint32_t idx = pos >= 0 ? bi[pos] : 0u;
    if (packed) { packed[ki] = val; packed[k + ki] = (float)idx; }
    else { a.values_out[ki] = val; a.indices_out[ki] = idx; }
  }
}

static bool shape_ok(int ncols, int k, int chunk_size, int nblocks) {
  return ncols > 0 && k >= 1 && k <= MAX_K && chunk_size >= 1 && chunk_size <= NT * MAXV && nblocks >= 1 && (long long)nblocks * chunk_size >= ncols;
}
static void run(const float *input, const float *inv_temperatures, float inv_temperature, float *block_values, uint32_t *block_indices, float *block_maxes,
                float *block_sums, float *packed_out, float *values_out, uint32_t *indices_out, float *softmax_info_out, int nrows, int ncols, int k,
                int chunk_size, int nblocks, int64_t stream) {
  if (!shape_ok(ncols, k, chunk_size, nblocks) || nrows < 1) return;  // the reference's host wrapper validates before it calls (ops.rs:699-731)
  hipStream_t s = (hipStream_t)stream;
  Stage1Args a1{input, block_values, block_indices, block_maxes, block_sums, inv_temperatures, inv_temperature, ncols, k, chunk_size, nblocks};
  const size_t heads_bytes = ((size_t)nblocks * sizeof(int) + 7) & ~(size_t)7;
  if (heads_bytes > 56 * 1024) return;  // > 14 k chunks (a 29 M-token vocabulary at the reference's chunk size): outside this kernel
  const int depth = (int)std::min<size_t>((size_t)k, (60 * 1024 - heads_bytes) / 8 / (size_t)nblocks);  // keys staged per list (60 KiB of LDS in all; 0 = read from memory)
  Stage2Args a2{block_values, block_indices, block_maxes, block_sums, packed_out, values_out, indices_out, softmax_info_out, nblocks, k, depth};
  const size_t lds2 = heads_bytes + (size_t)nblocks * depth * 8;
  hipLaunchKernelGGL(topk_stage1_kernel, dim3(nblocks, nrows), dim3(NT), 0, s, a1);  // the row is the block index: a single row is a grid of 1 in that dimension
  hipLaunchKernelGGL(topk_stage2_kernel, dim3(nrows), dim3(NT), lds2, s, a2);
}

// ---------------------------------------------------------------- greedy: top1_large_f32_packed[_batched] (sort.cu:1825-1912, 2071-2143, 2207-2238)
// stage 1: per chunk the largest logit and its (lowest) index; a chunk that holds a NaN reports (NaN, 0); no finite or +inf value -> (-inf, 0).
// stage 2: per row the best chunk (lowest position on ties); any NaN chunk -> token id UINT32_MAX and packed (NaN, NaN); nothing selectable -> token 0.
struct Top1Args {
  const float *input;
  float *block_values;
  uint32_t *block_indices;
  float *packed_out;
  uint32_t *token_ids_out;
  int ncols, chunk_size, nblocks;
};
// block-wide (key, value) arg-max + NaN flag: returns in thread 0
__device__ __forceinline__ void block_argmax(unsigned long long best, float val, bool nan, unsigned long long &okey, float &oval, bool &onan) {
  __shared__ unsigned long long s_k[4];
  __shared__ float s_v[4];
  __shared__ int s_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long w = wave_max_u64(best);
  const bool any_nan = __ballot(nan) != 0ull;
  if (w != 0ull && best == w) { s_k[wave] = w; s_v[wave] = val; }  // keys carry the position: one lane
  if (w == 0ull && lane == 0) { s_k[wave] = 0ull; s_v[wave] = -INFINITY; }
  if (lane == 0) s_n[wave] = any_nan;
  __syncthreads();
  okey = 0ull; oval = -INFINITY; onan = false;
  if (tid == 0) {
    for (int i = 0; i < 4; ++i) {
      if (s_k[i] > okey) { okey = s_k[i]; oval = s_v[i]; }
      onan = onan || s_n[i] != 0;
    }
  }
  __syncthreads();
}
__global__ void __launch_bounds__(NT) top1_stage1_kernel(Top1Args a) {
  const int tid = threadIdx.x, chunk = blockIdx.x;
  const size_t row = blockIdx.y;
  const float *input = a.input + row * (size_t)a.ncols;
  const int start = chunk * a.chunk_size, end = min(start + a.chunk_size, a.ncols);
  unsigned long long best = 0ull;
  float val = -INFINITY;
  bool nan = false;
  for (int idx = start + tid; idx < end; idx += NT) {
    const float c = input[idx];
    if (c != c) nan = true;
    const unsigned long long key = key_of(c, (unsigned)idx);
    if (key > best) { best = key; val = c; }
  }
  unsigned long long k; float v; bool n;
  block_argmax(best, val, nan, k, v, n);
  if (tid == 0) {
    a.block_values[row * a.nblocks + chunk] = n ? NAN : v;
    a.block_indices[row * a.nblocks + chunk] = n || k == 0ull ? 0u : idx_of(k);
  }
}
__global__ void __launch_bounds__(NT) top1_stage2_kernel(Top1Args a) {
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const float *bv = a.block_values + row * (size_t)a.nblocks;
  const uint32_t *bi = a.block_indices + row * (size_t)a.nblocks;
  unsigned long long best = 0ull;
  float val = -INFINITY;
  bool nan = false;
  for (int pos = tid; pos < a.nblocks; pos += NT) {
    const float c = bv[pos];
    if (c != c) nan = true;
    const unsigned long long key = key_of(c, (unsigned)pos);
    if (key > best) { best = key; val = c; }
  }
  unsigned long long k; float v; bool n;
  block_argmax(best, val, nan, k, v, n);
  if (tid == 0) {
    const uint32_t token = n ? 0xffffffffu : (k != 0ull ? bi[idx_of(k)] : 0u);
    if (a.packed_out) { a.packed_out[row * 2] = n ? NAN : v; a.packed_out[row * 2 + 1] = n ? NAN : (float)token; }
    if (a.token_ids_out) a.token_ids_out[row] = token;
  }
}
static void run_top1(const float *input, float *block_values, uint32_t *block_indices, float *packed_out, uint32_t *token_ids_out, int nrows, int ncols, int chunk_size,
                     int nblocks, int64_t stream) {
  if (ncols <= 0 || chunk_size <= 0 || nblocks <= 0 || nrows <= 0 || (long long)nblocks * chunk_size < ncols) return;
  hipStream_t s = (hipStream_t)stream;
  Top1Args a{input, block_values, block_indices, packed_out, token_ids_out, ncols, chunk_size, nblocks};
  hipLaunchKernelGGL(top1_stage1_kernel, dim3(nblocks, nrows), dim3(NT), 0, s, a);
  hipLaunchKernelGGL(top1_stage2_kernel, dim3(nrows), dim3(NT), 0, s, a);
}

// ---------------------------------------------------------------- temperature sampling over the whole row: categorical_large_f32_packed_batched
// (the reference's symbol: ffi.rs:666, sort.cu:1825-2069, 2240-2257; callers ops.rs:1347-1500, sampler.rs:649-652, 744-764).  One draw per row from softmax(x * invT) by
// inverting the cumulative distribution at the caller's uniform -- no top-k cut, nothing leaves the device but (token, logprob).
// stage 1, one workgroup per chunk: block_values = the chunk's largest raw logit (NaN if it holds one, -inf if nothing is above -inf), block_sums = the chunk's
//   sum of expf(x * invT - block_value * invT) -- the chunk is read ONCE into registers, max and sum both come from them; the sum IS top-k stage 1's (chunk_softmax_share).
// stage 2, one workgroup per row, opens with row_preamble: gmax = max_b block_values * invT; the chunk masses block_sums[b] * expf(block_values[b] * invT - gmax) computed once by all
//   threads, added in chunk order by thread 0 (running sums kept: the chunk that holds the target is a binary search over them); then the selected chunk, each thread
//   owning a CONTIGUOUS run of ceil(chunk_size / 256) tokens: thread-local running sums, an inclusive scan of the thread totals across the lanes (DPP row rotates +
//   v_readlane), the four wave totals through LDS with one barrier, and every thread tests its own tokens only.  Any chunk_size in 1..4096.
struct CatArgs {
  const float *input, *inv_temperatures, *uniforms;
  float *block_values, *block_sums, *packed_out;
  int ncols, chunk_size, nblocks;
};
constexpr int CAT_MAXB = 4096;  // running chunk masses kept in LDS; the chunks beyond (vocabularies > 8 M tokens at chunk_size 2048) are recomputed by the walk

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ void __launch_bounds__(NT) cat_stage1_kernel(CatArgs a) {
  const int tid = threadIdx.x, chunk = blockIdx.x;
  const size_t row = blockIdx.y;
  const float *input = a.input + row * (size_t)a.ncols;
  const float inv_t = a.inv_temperatures[row];
  const long long start = (long long)chunk * a.chunk_size, left = (long long)a.ncols - start;
  const int width = left <= 0 ? 0 : (left < a.chunk_size ? (int)left : a.chunk_size);
  float v[MAXV];
  load_chunk(input + start, width, v);
  float m = -INFINITY;
  bool nan = false, any_nan;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    if (v[j] != v[j]) nan = true;
    else m = fmaxf(m, v[j]);
  }
  m = block_max_nan<NT / 64>(m, nan, any_nan);
  const float block_value = any_nan ? NAN : m;
  const float block_sum = chunk_softmax_share(v, width, inv_t, block_value * inv_t, block_value == -INFINITY);
  if (tid == 0) {
    a.block_values[row * a.nblocks + chunk] = block_value;
    a.block_sums[row * a.nblocks + chunk] = block_sum;
  }
}

// inclusive / exclusive prefix sums of one value per lane over the wave, and the wave's total: a Hillis-Steele scan inside each row of 16 lanes on DPP row
// rotates (a lane that would wrap around adds nothing), then the three row totals through v_readlane.  excl(l) == incl(l - 1) bit for bit.
template <int N> __device__ __forceinline__ float row_ror_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + N, 0xf, 0xf, false));
}
__device__ __forceinline__ void wave_scan_f32(float v, float &excl, float &total) {
  const int lane = threadIdx.x & 63, i = lane & 15, r = lane >> 4;
  float t;
  t = row_ror_f32<1>(v); if (i >= 1) v += t;
  t = row_ror_f32<2>(v); if (i >= 2) v += t;
  t = row_ror_f32<4>(v); if (i >= 4) v += t;
  t = row_ror_f32<8>(v); if (i >= 8) v += t;
  t = row_ror_f32<1>(v);
  const float e = i >= 1 ? t : 0.0f;  // exclusive inside the row
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 15)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 47)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
  const float o1 = r0, o2 = r0 + r1, o3 = o2 + r2;
  const float off = r == 0 ? 0.0f : (r == 1 ? o1 : (r == 2 ? o2 : o3));
  excl = r == 0 ? e : off + e;
  total = o3 + r3;
}

// ---- the row preamble of both draws, for a workgroup of NTH threads over stage 1's workspace row (bv = chunk maxima, bs = chunk sums):
//   gmax = max_b bv[b] * inv_t in every thread (NaN if a chunk reports one);
//   the mass of chunk b under gmax is chunk_mass(b); all threads stage the first CAT_MAXB of them in s_cum, then THREAD 0 ALONE adds them in ascending chunk index
//   (the chunks beyond CAT_MAXB recomputed on the way) and, with RUNNING_SUMS, leaves the running sums in s_cum (the categorical draw bisects them; the nucleus draw
//   has no use for them, and the store after every load keeps the loop from running its LDS loads ahead: measured, profiles/sampling_refactor.md) -- the draws' denom
//   is this sum and no other;
//   `usable` = the row can be drawn from: inv_t and u in range, gmax and denom finite, denom > 0.
// denom and usable are valid in thread 0 only, and no barrier follows thread 0's loop: the caller publishes what its other threads need.
__device__ __forceinline__ float chunk_mass(const float *bv, const float *bs, int b, float inv_t, float gmax) { return bs[b] * expf(bv[b] * inv_t - gmax); }
template <int NTH, bool RUNNING_SUMS>
__device__ __forceinline__ float row_preamble(const float *bv, const float *bs, int nb, float inv_t, float u, float *s_cum /* LDS [CAT_MAXB] */, float &denom, bool &usable) {
  const int tid = threadIdx.x;
  float m = -INFINITY;
  bool nan = false, any_nan;
  for (int b = tid; b < nb; b += NTH) {
    const float c = bv[b];
    if (c != c) nan = true;
    else m = fmaxf(m, c);
  }
  m = block_max_nan<NTH / 64>(m, nan, any_nan);
  const float gmax = any_nan ? NAN : m * inv_t;
  for (int b = tid; b < nb && b < CAT_MAXB; b += NTH) s_cum[b] = chunk_mass(bv, bs, b, inv_t, gmax);
  __syncthreads();
  denom = 0.0f;
  usable = false;
  if (tid == 0) {
    float cum = 0.0f;
    for (int b = 0; b < nb; ++b) {
      cum += b < CAT_MAXB ? s_cum[b] : chunk_mass(bv, bs, b, inv_t, gmax);
      if (RUNNING_SUMS && b < CAT_MAXB) s_cum[b] = cum;
    }
    denom = cum;
    usable = inv_t > 0.0f && finite_f32(inv_t) && u >= 0.0f && u < 1.0f && finite_f32(gmax) && denom > 0.0f && finite_f32(denom);
  }
  return gmax;
}
// an unusable row: n NaNs (categorical_token / nucleus_token on the host refuse them)
__device__ __forceinline__ void store_nan_row(float *packed, int n) {
  for (int i = 0; i < n; ++i) packed[i] = NAN;
}

// ---- the inversion of running chunk sums at a uniform, shared by cat_stage2_kernel and the speculative verifier below (all threads call; the token is valid in
// thread 0, -1 = no token).  `s_cum` holds the running sums of the first min(nb, CAT_MAXB) chunk masses, `denom` their total over all nb chunks (thread 0), mass(b) gives
// the mass of a chunk beyond the staged ones, weight(i) the weight of token i.  Thread 0 picks the chunk by bisection, then each thread owns a CONTIGUOUS run of tokens of it.
template <class Mass, class Weight>
__device__ __forceinline__ int invert_running_sums(bool usable, float u, float denom, const float *s_cum, int nb, int chunk_size, int ncols, Mass mass, Weight weight) {
  __shared__ float s_wtot[4], s_wlast[4];
  __shared__ int s_wfirst[4];
  __shared__ float s_target;
  __shared__ int s_sel;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- thread 0: the target, the chunk that holds it
  if (tid == 0) {
    int sel = -1;
    float target = NAN;
    if (usable) {
      target = fminf(u * denom, nextafterf(denom, -INFINITY));
      const int nl = nb < CAT_MAXB ? nb : CAT_MAXB;
      float before = 0.0f;
      if (target < s_cum[nl - 1]) {  // the running sums never decrease: the first one above the target by bisection
        int lo = 0, hi = nl - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (target < s_cum[mid]) hi = mid;
          else lo = mid + 1;
        }
        sel = lo;
        before = lo > 0 ? s_cum[lo - 1] : 0.0f;
      } else {  // beyond the staged chunks: walk on
        float c = s_cum[nl - 1];
        for (int b = nl; b < nb; ++b) {
          const float next = c + mass(b);
          if (target < next) { sel = b; before = c; break; }
          c = next;
        }
      }
      target -= before;
    }
    s_sel = sel;
    s_target = target;
  }
  __syncthreads();
  const int sel = s_sel;
  if (sel < 0) return -1;
  const float target = s_target;
  // ---- the selected chunk: thread t owns the tokens [t * per, t * per + per)
  const long long start = (long long)sel * chunk_size, left = (long long)ncols - start;
  const int width = left < chunk_size ? (int)left : chunk_size;
  const int per = (chunk_size + NT - 1) / NT, first = tid * per;
  float w[MAXV], run[MAXV];  // weights, and their running sums inside the thread
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    const int local = first + j;
    w[j] = (j < per && local < width) ? weight(start + local) : 0.0f;
    acc += w[j];
    run[j] = acc;
  }
  float excl, wave_total;
  wave_scan_f32(acc, excl, wave_total);
  if (lane == 0) s_wtot[wave] = wave_total;
  __syncthreads();
  const float t0 = s_wtot[0], t01 = t0 + s_wtot[1], t012 = t01 + s_wtot[2];
  const float base = wave == 0 ? excl : (wave == 1 ? t0 : (wave == 2 ? t01 : t012)) + excl;
  // the lowest token with weight > 0 whose inclusive cumulative weight exceeds the target; and the last token with weight > 0, for when rounding leaves none
  int hit = -1, last = -1;
#pragma unroll
  for (int j = MAXV - 1; j >= 0; --j) {
    if (w[j] > 0.0f) {
      if (last < 0) last = first + j;
      if (base + run[j] > target) hit = first + j;
    }
  }
  const unsigned long long hits = __ballot(hit >= 0);  // threads own ascending runs: the lowest lane with a hit holds the wave's lowest token
  const int first_lane = hits ? __ffsll((long long)hits) - 1 : 0;
  const int wave_first = __builtin_amdgcn_readlane(hit, first_lane);
  const float wave_last = wave_max((float)last);  // < 4096: exact in f32
  if (lane == 0) { s_wfirst[wave] = hits ? wave_first : -1; s_wlast[wave] = wave_last; }
  __syncthreads();
  int token = -1;
  if (tid == 0) {
    for (int i = 3; i >= 0; --i) if (s_wfirst[i] >= 0) token = s_wfirst[i];
    if (token < 0) token = (int)fmaxf(fmaxf(s_wlast[0], s_wlast[1]), fmaxf(s_wlast[2], s_wlast[3]));
    if (token >= 0) token += (int)start;  // otherwise unreachable while the chunk's mass is > 0
  }
  return token;
}

__global__ void __launch_bounds__(NT) cat_stage2_kernel(CatArgs a) {
  __shared__ float s_cum[CAT_MAXB];  // chunk masses, then their running sums
  const int tid = threadIdx.x, nb = a.nblocks;
  const size_t row = blockIdx.x;
  const float *input = a.input + row * (size_t)a.ncols;
  const float *bv = a.block_values + row * (size_t)nb, *bs = a.block_sums + row * (size_t)nb;
  float *packed = a.packed_out + row * 2;
  const float inv_t = a.inv_temperatures[row], u = a.uniforms[row];
  float denom;
  bool usable;
  const float gmax = row_preamble<NT, true>(bv, bs, nb, inv_t, u, s_cum, denom, usable);
  const int token = invert_running_sums(usable, u, denom, s_cum, nb, a.chunk_size, a.ncols, [&](int b) { return chunk_mass(bv, bs, b, inv_t, gmax); },
                                        [&](long long i) { return expf(input[i] * inv_t - gmax); });
  if (tid == 0) {
    if (token < 0) { store_nan_row(packed, 2); return; }
    packed[0] = (float)token;
    packed[1] = input[token] * inv_t - gmax - logf(denom);
  }
}

static bool draw_shape_ok(int nrows, int ncols, int chunk_size, int nblocks) {  // the refusals of both draws: their stage 1 is the same launch
  return nrows >= 1 && ncols >= 1 && chunk_size >= 1 && chunk_size <= NT * MAXV && (long long)nblocks * chunk_size >= ncols;
}
static void run_categorical(const float *input, const float *inv_temperatures, const float *uniforms, float *block_values, float *block_sums, float *packed_out, int nrows,
                            int ncols, int chunk_size, int nblocks, int64_t stream) {
  if (!draw_shape_ok(nrows, ncols, chunk_size, nblocks)) return;
  hipStream_t s = (hipStream_t)stream;
  CatArgs a{input, inv_temperatures, uniforms, block_values, block_sums, packed_out, ncols, chunk_size, nblocks};
  hipLaunchKernelGGL(cat_stage1_kernel, dim3(nblocks, nrows), dim3(NT), 0, s, a);
  hipLaunchKernelGGL(cat_stage2_kernel, dim3(nrows), dim3(NT), 0, s, a);
}

// ---------------------------------------------------------------- top-p / min-p over the whole row: mrs_nucleus_large_f32_packed_batched (no reference counterpart:
// with top-k unset and a cut active the reference leaves the device, sampler.rs:649-655, and sorts the whole vocabulary on the host, sampler.rs:1605-1662).
// stage 1 is cat_stage1_kernel as it is, so denom is the categorical denom.  stage 2, one workgroup of 1024 threads per row:
//   gmax, denom (chunk order, thread 0) and the row's validity from row_preamble, on 16 waves;
//   every mass after that is a FIXED-POINT INTEGER, q_i = (u64)(expf(x_i * invT - gmax) * 2^39): integer adds are exact in any order, so the histogram below may use
//   LDS atomics, and x*, the kept mass and the drawn token are functions of the row's f32 weights alone -- bit-identical whatever the launch, the batch row or the
//   neighbours are.  (2^39, not 2^40: 2^24 tokens of weight 1 sum to 2^63 and cannot wrap; the largest weight is exactly 1 under -ffp-contract=off and 1 to within rounding otherwise.  The truncation costs at most ncols * 2^-39 of absolute mass.)
//   top-p: x* = the logit at which the mass of the strictly greater logits first stays below top_p * Q (Q = sum q_i), found by a radix select over the
//   order-preserving 32-bit key of the logit, 4 passes of 8 bits: a pass streams the row, adds q_i of the tokens that match the prefix into its wave's own 256-bin
//   histogram (16 copies, 32 KiB), the copies are summed, and wave 0 walks the bins from the top (4 bins per lane + a lane scan) to the bin where the cumulative mass
//   reaches the cutoff.  All logits equal to x* are kept (the reference keeps those its unstable sort puts first).  min-p: w_i > min_p on the f32 weight.
//   draw: one pass for the kept mass of each wave's 1/16 of the row, then the 1024 threads share the segment that holds target = min((u64)(u * K), K - 1):
//   contiguous runs per thread, an integer scan, the lowest kept token whose inclusive cumulative mass exceeds the target.  K > target, so a token always exists.
// No barrier sits inside a per-token loop; no float is added in an order the hardware picks.
struct NucArgs {
  const float *input, *inv_temperatures, *uniforms, *top_ps, *min_ps;
  const float *block_values, *block_sums;
  float *packed_out;  // [rows][4] = token, logprob under the full softmax, x* (-inf without top-p), kept mass / total mass
  int ncols, chunk_size, nblocks;
};
constexpr int NUC_NT = 1024, NUC_WAVES = NUC_NT / 64, NUC_UNROLL = 8;
typedef unsigned long long u64;

__device__ __forceinline__ u64 fixed_mass(float w) { return (u64)(w * 549755813888.0f); }  // 2^39: the product is exact, the conversion truncates
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ u64 wave_scan_u64(u64 v) {  // inclusive
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl(v, (lane - d) & 63, 64);
    if (lane >= d) v += o;
  }
  return v;
}

__global__ void __launch_bounds__(NUC_NT) nuc_stage2_kernel(NucArgs a) {
  __shared__ u64 s_hist[NUC_WAVES][256];
  __shared__ float s_cum[CAT_MAXB];  // the preamble's staging of the chunk masses
  __shared__ u64 s_wkept[NUC_WAVES], s_wall[NUC_WAVES], s_wscan[NUC_WAVES];
  __shared__ float s_denom;
  __shared__ int s_ok, s_digit;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nb = a.nblocks, n = a.ncols;
  const size_t row = blockIdx.x;
  const float *input = a.input + row * (size_t)n;
  const float *bv = a.block_values + row * (size_t)nb, *bs = a.block_sums + row * (size_t)nb;
  float *packed = a.packed_out + row * 4;
  const float inv_t = a.inv_temperatures[row], u = a.uniforms[row], top_p = a.top_ps[row], min_p = a.min_ps[row];
  const bool cut_p = top_p > 0.0f && top_p < 1.0f, cut_m = min_p > 0.0f && min_p < 1.0f;  // NaN: no cut
  float denom;
  bool usable;
  const float gmax = row_preamble<NUC_NT, false>(bv, bs, nb, inv_t, u, s_cum, denom, usable);
  if (tid == 0) {
    s_denom = denom;
    s_ok = usable ? 1 : 0;
    if (!usable) store_nan_row(packed, 4);
  }
  __syncthreads();
  if (!s_ok) return;
  auto weight = [&](float x) { return expf(x * inv_t - gmax); };
  // ---- top-p: the threshold key, 8 bits a pass from the top
  unsigned kstar = 0u;  // every key is >= 0: no top-p cut
  double cut = 0.0;
  u64 above = 0ull;
  if (cut_p) {
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int i = tid; i < NUC_WAVES * 256; i += NUC_NT) (&s_hist[0][0])[i] = 0ull;
      __syncthreads();
      for (long long base = tid; base < n; base += NUC_UNROLL * NUC_NT) {  // NUC_UNROLL loads in flight: one workgroup streams the row, and a load is a trip to L2
        float xs[NUC_UNROLL];
#pragma unroll
        for (int j = 0; j < NUC_UNROLL; ++j) {
          const long long i = base + (long long)j * NUC_NT;
          xs[j] = i < n ? input[i] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NUC_UNROLL; ++j) {
          const unsigned key = order_key(xs[j]);
          if (base + (long long)j * NUC_NT < n && (pass == 0 || (key >> (shift + 8)) == (kstar >> (shift + 8)))) {
            const u64 q = fixed_mass(weight(xs[j]));
            if (q != 0ull) atomicAdd(&s_hist[wave][(key >> shift) & 255u], q);
          }
        }
      }
      __syncthreads();
      if (tid < 256) {
        u64 t = 0ull;
        for (int w = 0; w < NUC_WAVES; ++w) t += s_hist[w][tid];
        s_hist[0][tid] = t;  // only this thread reads or writes column `tid`
      }
      __syncthreads();
      if (wave == 0) {  // lane l owns the bins 255 - 4l .. 252 - 4l, walked downwards; `cut` and `above` live in wave 0's registers across the passes
        u64 t[4], local = 0ull;
#pragma unroll
        for (int j = 0; j < 4; ++j) { t[j] = s_hist[0][255 - 4 * lane - j]; local += t[j]; }
        const u64 incl = wave_scan_u64(local);
        if (pass == 0) cut = (double)top_p * (double)__shfl(incl, 63, 64);  // top_p * Q, Q = the row's whole mass; > 0: the arg-max alone weighs about 2^39
        u64 cum = above + (incl - local);
        int hit = -1;
        u64 hit_above = 0ull;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (hit < 0 && t[j] != 0ull && (double)(cum + t[j]) >= cut) { hit = 255 - 4 * lane - j; hit_above = cum; }
          cum += t[j];
        }
        const unsigned long long hits = __ballot(hit >= 0);
        const int first_lane = hits ? __ffsll((long long)hits) - 1 : 0;
        above = __shfl(hit_above, first_lane, 64);  // the mass strictly above the chosen bin: stays below the cutoff
        const int digit = __shfl(hit, first_lane, 64);
        if (lane == 0) s_digit = hits ? digit : -1;
      }
      __syncthreads();
      const int digit = s_digit;
      if (digit < 0) {  // unreachable: the cumulative mass ends at the bin mass the previous pass selected, which had reached the cutoff
        if (tid == 0) store_nan_row(packed, 4);
        return;
      }
      kstar |= (unsigned)digit << shift;
    }
  }
  // ---- kept mass and total mass of each wave's sixteenth of the row
  auto kept_mass = [&](float x) -> u64 {
    const float w = weight(x);
    return (order_key(x) >= kstar && (!cut_m || w > min_p)) ? fixed_mass(w) : 0ull;
  };
  const long long seg = ((long long)n + NUC_WAVES - 1) / NUC_WAVES;
  {
    const long long lo = wave * seg, hi = lo + seg < n ? lo + seg : n;
    u64 kq = 0ull, tq = 0ull;
    for (long long base = lo + lane; base < hi; base += NUC_UNROLL * 64) {
      float xs[NUC_UNROLL];
#pragma unroll
      for (int j = 0; j < NUC_UNROLL; ++j) {
        const long long i = base + j * 64;
        xs[j] = i < hi ? input[i] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < NUC_UNROLL; ++j) {
        if (base + j * 64 < hi) {
          const float w = weight(xs[j]);
          const u64 q = fixed_mass(w);
          tq += q;
          if (order_key(xs[j]) >= kstar && (!cut_m || w > min_p)) kq += q;
        }
      }
    }
    kq = wave_sum_u64(kq);
    tq = wave_sum_u64(tq);
    if (lane == 0) { s_wkept[wave] = kq; s_wall[wave] = tq; }
  }
  __syncthreads();
  u64 kept = 0ull, all = 0ull, before = 0ull;
  for (int w = 0; w < NUC_WAVES; ++w) { kept += s_wkept[w]; all += s_wall[w]; }
  if (kept == 0ull) {  // unreachable: the arg-max has weight 1 (to within rounding in a contracted build) and passes both cuts
    if (tid == 0) store_nan_row(packed, 4);
    return;
  }
  u64 target = (u64)((double)u * (double)kept);
  if (target >= kept) target = kept - 1ull;
  int sel = NUC_WAVES - 1;
  for (int w = 0; w < NUC_WAVES; ++w) {
    if (before + s_wkept[w] > target) { sel = w; break; }
    before += s_wkept[w];
  }
  target -= before;  // < s_wkept[sel]
  // ---- the selected sixteenth: thread t owns the tokens [lo + t * per, lo + t * per + per)
  const long long lo = sel * seg, hi = lo + seg < n ? lo + seg : n;
  const long long per = (seg + NUC_NT - 1) / NUC_NT, first = lo + tid * per, last = first + per < hi ? first + per : hi;
  u64 mine = 0ull;
  for (long long i = first; i < last; ++i) mine += kept_mass(input[i]);
  const u64 incl = wave_scan_u64(mine);
  if (lane == 63) s_wscan[wave] = incl;
  __syncthreads();
  u64 run = incl - mine;
  for (int w = 0; w < wave; ++w) run += s_wscan[w];
  // the lowest kept token whose inclusive cumulative mass exceeds the target: a token of mass 0 never moves the sum and is never returned
  long long hit = -1;
  if (run <= target && run + mine > target)
    for (long long i = first; i < last && hit < 0; ++i) {
      run += kept_mass(input[i]);
      if (run > target) hit = i;
    }
  if (hit >= 0) {  // exactly one thread of the workgroup holds the crossing: 0 <= target < the segment's kept mass, all integers
    const float x = input[hit];
    packed[0] = (float)hit;
    packed[1] = x * inv_t - gmax - logf(s_denom);
    packed[2] = cut_p ? order_key_value(kstar) : -INFINITY;
    packed[3] = (float)((double)kept / (double)all);
  }
}

static void run_nucleus(const float *input, const float *inv_temperatures, const float *uniforms, const float *top_ps, const float *min_ps, float *block_values,
                        float *block_sums, float *packed_out, int nrows, int ncols, int chunk_size, int nblocks, int64_t stream) {
  if (!draw_shape_ok(nrows, ncols, chunk_size, nblocks)) return;
  hipStream_t s = (hipStream_t)stream;
  CatArgs a1{input, inv_temperatures, uniforms, block_values, block_sums, nullptr, ncols, chunk_size, nblocks};
  NucArgs a2{input, inv_temperatures, uniforms, top_ps, min_ps, block_values, block_sums, packed_out, ncols, chunk_size, nblocks};
  hipLaunchKernelGGL(cat_stage1_kernel, dim3(nblocks, nrows), dim3(NT), 0, s, a1);
  hipLaunchKernelGGL(nuc_stage2_kernel, dim3(nrows), dim3(NUC_NT), 0, s, a2);
}

// ---------------------------------------------------------------- speculative decoding, the verifier: mrs_spec_verify_f32_batched (no reference symbol: the reference
// runs the accept loop on the host over full-vocabulary probability vectors -- mistralrs-core/src/speculative/verifier.rs:44-115 greedy verification with a batched
// device top-1, :200-290 the accept loop, :339-473 the stochastic rule).  Here the round of EVERY sequence is one launch group and nothing leaves the device but
// (n_accepted, out_tokens).  Sequence s owns the rows seq_rows[s] .. seq_rows[s + 1] of target_logits: row i judges draft i, the last row is the bonus row.
//   spec_stage1_kernel   grid (chunks, rows): the chunk in registers once (load_chunk); its greedy key (pack_max: largest value, lowest index, -0.0 == +0.0), its maximum
//                        with the NaN flag (block_max_nan) and, in temperature mode, its share of the normaliser (chunk_softmax_share) for p -- cat_stage1_kernel's
//                        values bit for bit -- and the same pair for q when the proposer handed over logits.                       (verifier.rs:44-115, 339-380)
//   spec_decide_kernel   one workgroup per sequence walks the rows IN ORDER and stops at the first that ends the round, so later rows are never read (they may hold NaN).
//                        greedy: winner == draft.  temperature: row_preamble for p (and q), p_d = w_p / denom_p, q_d likewise (1 without draft logits),
//                        accept = q_d > 0 ? min(1, p_d / q_d) : (p_d > 0 ? 1 : 0), accepted iff u0 < accept.  All accepted: the bonus row is drawn here, by
//                        row_preamble + invert_running_sums exactly as cat_stage2_kernel does at u1.  A rejection leaves a record for the two launches below.  (verifier.rs:200-290)
//   spec_residual_kernel grid (chunks, sequences): only the workgroups of a sequence with a record stay; chunk mass of max(p - q, 0).              (verifier.rs:381-440)
//   spec_resolve_kernel  one workgroup per sequence with a record: running residual sums in chunk order by thread 0, inversion at u1; a residual sum that is not positive
//                        falls back to the draw from p.                                                                                           (verifier.rs:441-473)
// No atomics and no float added in an order the hardware picks: the result is a function of the sequence's rows alone, whatever its neighbours in the launch are.
struct SpecRec {  // left by spec_decide_kernel for a sequence whose round ends in a rejection
  int32_t row;    // the rejected row (global index), -1: nothing left to do
  int32_t draft, n_acc;
  float gp, dp, gq, dq;  // gmax and denom of p and of q on that row
  int32_t pad;
};
struct SpecArgs {
  const float *target, *draft;  // draft == NULL: a deterministic proposer, q is one-hot on the draft
  const int32_t *draft_ids, *seq_rows, *modes;
  const float *inv_temperatures, *uniforms;
  unsigned long long *keys;     // [rows][nb]
  float *bvp, *bsp, *bvq, *bsq; // [rows][nb]
  float *res;                   // [nseq][nb]
  SpecRec *rec;                 // [nseq]
  int32_t *n_accepted, *out_tokens;
  int nseq, total_rows, ncols, chunk_size, nblocks;
};
constexpr int SPEC_MAX_ROWS = 8, SPEC_GREEDY = 0, SPEC_TEMPERATURE = 1;

// (== ext_decode.hip pack_max, the key of mrs_sample_greedy_advance)
__device__ __forceinline__ unsigned long long pack_max(float v, int idx) {
  unsigned u = __float_as_uint(v);
  u = u == 0x80000000u ? 0u : u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned)(0x7fffffff - idx);
}
__device__ __forceinline__ int spec_seq_of_row(const int32_t *seq_rows, int nseq, int row) {  // the last s with seq_rows[s] <= row
  int lo = 0, hi = nseq - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seq_rows[mid] <= row) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// max(p - q, 0) of one token; without draft logits q is one-hot on the draft, whose residual is 0 by definition (never p - 1 rounded)
__device__ __forceinline__ float spec_residual(float xp, float xq, bool has_q, bool is_draft, float inv_t, const SpecRec &r) {
  if (!has_q) return is_draft ? 0.0f : expf(xp * inv_t - r.gp) / r.dp;
  return fmaxf(expf(xp * inv_t - r.gp) / r.dp - expf(xq * inv_t - r.gq) / r.dq, 0.0f);
}

__global__ void __launch_bounds__(NT) spec_stage1_kernel(SpecArgs a) {
  __shared__ unsigned long long s_key[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x, row = blockIdx.y, nb = a.nblocks;
  const int s = spec_seq_of_row(a.seq_rows, a.nseq, row);
  const int mode = a.modes[s];
  const float inv_t = a.inv_temperatures[s];
  const long long start = (long long)chunk * a.chunk_size, left = (long long)a.ncols - start;
  const int width = left <= 0 ? 0 : (left < a.chunk_size ? (int)left : a.chunk_size);
  const size_t at = (size_t)row * nb + chunk;
  float v[MAXV];
  load_chunk(a.target + (size_t)row * a.ncols + start, width, v);
  unsigned long long best = 0ull;
  float m = -INFINITY;
  bool nan = false, any_nan;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    const int local = tid + j * NT;
    if (local < width) {
      const unsigned long long key = pack_max(v[j], (int)start + local);
      best = key > best ? key : best;
    }
    if (v[j] != v[j]) nan = true;
    else m = fmaxf(m, v[j]);
  }
  best = wave_max_u64(best);
  if (lane == 0) s_key[wave] = best;
  m = block_max_nan<NT / 64>(m, nan, any_nan);  // its barrier publishes s_key too
  const float bvp = any_nan ? NAN : m;
  if (tid == 0) {
    unsigned long long k = s_key[0];
    for (int i = 1; i < NT / 64; ++i) k = s_key[i] > k ? s_key[i] : k;
    a.keys[at] = k;
    a.bvp[at] = bvp;
  }
  if (mode != SPEC_TEMPERATURE) return;  // uniform over the workgroup
  const float bsp = chunk_softmax_share(v, width, inv_t, bvp * inv_t, bvp == -INFINITY);  // two barriers: block_max_nan's slots are free again below
  if (tid == 0) a.bsp[at] = bsp;
  if (!a.draft) return;
  load_chunk(a.draft + (size_t)row * a.ncols + start, width, v);
  m = -INFINITY;
  nan = false;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    if (v[j] != v[j]) nan = true;
    else m = fmaxf(m, v[j]);
  }
  m = block_max_nan<NT / 64>(m, nan, any_nan);
  const float bvq = any_nan ? NAN : m;
  const float bsq = chunk_softmax_share(v, width, inv_t, bvq * inv_t, bvq == -INFINITY);
  if (tid == 0) { a.bvq[at] = bvq; a.bsq[at] = bsq; }
}

__device__ __forceinline__ void spec_store_round(const SpecArgs &a, int s, int n_acc, int cont) {  // thread 0: the entries past the continuation read -1; n_acc < 0: all of them
  int32_t *out = a.out_tokens + (size_t)s * SPEC_MAX_ROWS;
  for (int i = n_acc < 0 ? 0 : n_acc + 1; i < SPEC_MAX_ROWS; ++i) out[i] = -1;
  if (n_acc >= 0) out[n_acc] = cont;
  a.n_accepted[s] = n_acc < 0 ? -1 : n_acc;
}

__global__ void __launch_bounds__(NT) spec_decide_kernel(SpecArgs a) {
  __shared__ float s_cum[CAT_MAXB];
  __shared__ unsigned long long s_k[NT / 64];
  __shared__ int s_n[NT / 64];
  __shared__ int s_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x, nb = a.nblocks;
  const int r0 = a.seq_rows[s], r1 = a.seq_rows[s + 1], n = r1 - r0 - 1, mode = a.modes[s];
  int32_t *out = a.out_tokens + (size_t)s * SPEC_MAX_ROWS;
  if (tid == 0) a.rec[s].row = -1;
  if (r0 < 0 || r1 > a.total_rows || n < 0 || n >= SPEC_MAX_ROWS || (mode != SPEC_GREEDY && mode != SPEC_TEMPERATURE)) {
    if (tid == 0) spec_store_round(a, s, -1, -1);
    return;
  }
  int acc = 0;
  if (mode == SPEC_GREEDY) {
    int cont = -1;
    for (int i = 0; i <= n && cont < 0; ++i) {
      const size_t row = (size_t)(r0 + i);
      unsigned long long best = 0ull;
      bool nan = false;
      for (int b = tid; b < nb; b += NT) {
        const unsigned long long k = a.keys[row * nb + b];
        const float c = a.bvp[row * nb + b];
        best = k > best ? k : best;
        if (c != c) nan = true;
      }
      best = wave_max_u64(best);
      const bool wave_nan = __ballot(nan) != 0ull;
      if (lane == 0) { s_k[wave] = best; s_n[wave] = wave_nan ? 1 : 0; }
      __syncthreads();
      unsigned long long k = 0ull;
      int nans = 0;
#pragma unroll
      for (int w = 0; w < NT / 64; ++w) { k = s_k[w] > k ? s_k[w] : k; nans |= s_n[w]; }
      __syncthreads();  // the slots are rewritten by the next row
      if (nans) { acc = -1; break; }  // a NaN in a row that decides: unusable
      const int winner = 0x7fffffff - (int)(k & 0xffffffffull);
      if (i < n && winner == a.draft_ids[row]) {
        if (tid == 0) out[i] = winner;
        ++acc;
      } else cont = winner;
    }
    if (tid == 0) spec_store_round(a, s, acc, cont);
    return;
  }
  const float inv_t = a.inv_temperatures[s];
  int state = 0;  // 0: every draft accepted, 1: a rejection (the record is written), 2: unusable
  for (int i = 0; i < n && state == 0; ++i) {
    const size_t row = (size_t)(r0 + i);
    const float u0 = a.uniforms[2 * row];
    float denom, gq = 0.0f, dq = 1.0f;
    bool usable;
    const float gp = row_preamble<NT, false>(a.bvp + row * nb, a.bsp + row * nb, nb, inv_t, u0, s_cum, denom, usable);
    const float dp = denom;
    bool ok = usable;
    __syncthreads();  // thread 0 has left s_cum
    if (a.draft) {
      gq = row_preamble<NT, false>(a.bvq + row * nb, a.bsq + row * nb, nb, inv_t, u0, s_cum, denom, usable);
      dq = denom;
      ok = ok && usable;
      __syncthreads();
    }
    if (tid == 0) {
      const int d = a.draft_ids[row];
      int flag = 2;
      if (ok && d >= 0 && d < a.ncols) {
        const float pd = expf(a.target[row * a.ncols + d] * inv_t - gp) / dp;
        const float qd = a.draft ? expf(a.draft[row * a.ncols + d] * inv_t - gq) / dq : 1.0f;
        const float accept = qd > 0.0f ? fminf(1.0f, pd / qd) : (pd > 0.0f ? 1.0f : 0.0f);
        flag = u0 < accept ? 0 : 1;  // accept == 0 rejects u0 == 0 too
        if (flag == 0) out[i] = d;
        else a.rec[s] = SpecRec{(int32_t)row, d, i, gp, dp, gq, dq, 0};
      }
      s_flag = flag;
    }
    __syncthreads();
    state = s_flag;
    __syncthreads();
    if (state == 0) ++acc;
  }
  if (state == 2) {
    if (tid == 0) spec_store_round(a, s, -1, -1);
    return;
  }
  if (state == 1) {  // the continuation comes from spec_resolve_kernel
    if (tid == 0) spec_store_round(a, s, acc, -1);
    return;
  }
  // every draft accepted (or none proposed): the bonus row is the categorical draw at u1, cat_stage2_kernel's arithmetic
  const size_t row = (size_t)(r0 + n);
  const float *input = a.target + row * a.ncols, *bv = a.bvp + row * nb, *bs = a.bsp + row * nb;
  const float u1 = a.uniforms[2 * row + 1];
  float denom;
  bool usable;
  const float gmax = row_preamble<NT, true>(bv, bs, nb, inv_t, u1, s_cum, denom, usable);
  const int token = invert_running_sums(usable, u1, denom, s_cum, nb, a.chunk_size, a.ncols, [&](int b) { return chunk_mass(bv, bs, b, inv_t, gmax); },
                                        [&](long long i) { return expf(input[i] * inv_t - gmax); });
  if (tid == 0) spec_store_round(a, s, token < 0 ? -1 : acc, token);
}

__global__ void __launch_bounds__(NT) spec_residual_kernel(SpecArgs a) {
  __shared__ float s_warp_sums[32];
  const int tid = threadIdx.x, chunk = blockIdx.x, s = blockIdx.y;
  const SpecRec r = a.rec[s];
  if (r.row < 0) return;  // every sequence whose round did not end in a rejection leaves at once
  const float inv_t = a.inv_temperatures[s];
  const long long start = (long long)chunk * a.chunk_size, left = (long long)a.ncols - start;
  const int width = left <= 0 ? 0 : (left < a.chunk_size ? (int)left : a.chunk_size);
  float v[MAXV], vq[MAXV];
  load_chunk(a.target + (size_t)r.row * a.ncols + start, width, v);
  if (a.draft) load_chunk(a.draft + (size_t)r.row * a.ncols + start, width, vq);
  float local_sum = 0.0f;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    const int local = tid + j * NT;
    if (local < width) local_sum += spec_residual(v[j], a.draft ? vq[j] : 0.0f, a.draft != nullptr, start + local == r.draft, inv_t, r);
  }
  const float mass = block_sum_ref_order(local_sum, s_warp_sums);
  if (tid == 0) a.res[(size_t)s * a.nblocks + chunk] = mass;
}

__global__ void __launch_bounds__(NT) spec_resolve_kernel(SpecArgs a) {
  __shared__ float s_cum[CAT_MAXB];
  __shared__ float s_total;
  __shared__ int s_residual;
  const int tid = threadIdx.x, s = blockIdx.x, nb = a.nblocks;
  const SpecRec r = a.rec[s];
  if (r.row < 0) return;
  const size_t row = (size_t)r.row;
  const float inv_t = a.inv_temperatures[s], u1 = a.uniforms[2 * row + 1];
  const float *res = a.res + (size_t)s * nb;
  const float *input = a.target + row * a.ncols, *dinput = a.draft ? a.draft + row * a.ncols : nullptr;
  for (int b = tid; b < nb && b < CAT_MAXB; b += NT) s_cum[b] = res[b];
  __syncthreads();
  if (tid == 0) {  // the residual masses in ascending chunk index, by one thread
    float cum = 0.0f;
    for (int b = 0; b < nb; ++b) {
      cum += b < CAT_MAXB ? s_cum[b] : res[b];
      if (b < CAT_MAXB) s_cum[b] = cum;
    }
    s_total = cum;
    s_residual = cum > 0.0f && finite_f32(cum) ? 1 : 0;
  }
  __syncthreads();
  int token;
  if (s_residual) {
    const float total = s_total;
    token = invert_running_sums(u1 >= 0.0f && u1 < 1.0f, u1, total, s_cum, nb, a.chunk_size, a.ncols, [&](int b) { return res[b]; },
                                [&](long long i) { return spec_residual(input[i], dinput ? dinput[i] : 0.0f, dinput != nullptr, i == r.draft, inv_t, r); });
  } else {  // p <= q everywhere: draw from p
    const float *bv = a.bvp + row * nb, *bs = a.bsp + row * nb;
    float denom;
    bool usable;
    const float gmax = row_preamble<NT, true>(bv, bs, nb, inv_t, u1, s_cum, denom, usable);
    token = invert_running_sums(usable, u1, denom, s_cum, nb, a.chunk_size, a.ncols, [&](int b) { return chunk_mass(bv, bs, b, inv_t, gmax); },
                                [&](long long i) { return expf(input[i] * inv_t - gmax); });
  }
  if (tid == 0) spec_store_round(a, s, token < 0 ? -1 : r.n_acc, token);
}

static size_t spec_align(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t spec_workspace_bytes(int total_rows, int nseq, int nblocks) {
  if (total_rows < 1 || nseq < 1 || nblocks < 1) return 0;
  const size_t cells = (size_t)total_rows * nblocks;
  return spec_align(cells * 8) + 4 * spec_align(cells * 4) + spec_align((size_t)nseq * nblocks * 4) + spec_align((size_t)nseq * sizeof(SpecRec));
}
static void run_spec_verify(const float *target, const float *draft, const int32_t *draft_ids, const int32_t *seq_rows, const int32_t *modes, const float *inv_temperatures,
                            const float *uniforms, void *workspace, size_t workspace_bytes, int32_t *n_accepted, int32_t *out_tokens, int nseq, int total_rows, int ncols,
                            int chunk_size, int nblocks, int64_t stream) {
  // rows are a grid dimension; a sequence has 1..8 rows (the kernels check each sequence's own count on the device)
  if (nseq < 1 || nseq > 65535 || total_rows < nseq || (long long)total_rows > (long long)SPEC_MAX_ROWS * nseq || total_rows > 65535) return;
  if (!draw_shape_ok(total_rows, ncols, chunk_size, nblocks) || !workspace || workspace_bytes < spec_workspace_bytes(total_rows, nseq, nblocks)) return;
  if ((uintptr_t)workspace & 7) return;
  const size_t cells = (size_t)total_rows * nblocks;
  char *w = (char *)workspace;
  SpecArgs a{target, draft, draft_ids, seq_rows, modes, inv_temperatures, uniforms};
  a.keys = (unsigned long long *)w; w += spec_align(cells * 8);
  a.bvp = (float *)w; w += spec_align(cells * 4);
  a.bsp = (float *)w; w += spec_align(cells * 4);
  a.bvq = (float *)w; w += spec_align(cells * 4);
  a.bsq = (float *)w; w += spec_align(cells * 4);
  a.res = (float *)w; w += spec_align((size_t)nseq * nblocks * 4);
  a.rec = (SpecRec *)w;
  a.n_accepted = n_accepted; a.out_tokens = out_tokens;
  a.nseq = nseq; a.total_rows = total_rows; a.ncols = ncols; a.chunk_size = chunk_size; a.nblocks = nblocks;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(spec_stage1_kernel, dim3(nblocks, total_rows), dim3(NT), 0, s, a);
  hipLaunchKernelGGL(spec_decide_kernel, dim3(nseq), dim3(NT), 0, s, a);
  hipLaunchKernelGGL(spec_residual_kernel, dim3(nblocks, nseq), dim3(NT), 0, s, a);
  hipLaunchKernelGGL(spec_resolve_kernel, dim3(nseq), dim3(NT), 0, s, a);
}

// ---------------------------------------------------------------- logits pre-processing of the sampler (sort.cu:8-110; callers sampler.rs:1113-1169)
// dst = x, then the listed tokens are updated in place: penalties (frequency / presence / repetition, counts from the context) or additive biases.
__global__ void __launch_bounds__(NT) copy_f32_kernel(const float *__restrict__ x, float *__restrict__ dst, int n) {
  const int i = (blockIdx.x * NT + threadIdx.x) * 4;
  if (i + 3 < n && ((((uintptr_t)x | (uintptr_t)dst) & 15) == 0)) *(float4 *)(dst + i) = *(const float4 *)(x + i);
  else
    for (int j = i; j < n && j < i + 4; ++j) dst[j] = x[j];
}
__global__ void __launch_bounds__(NT) sparse_penalties_kernel(float *__restrict__ logits, const uint32_t *__restrict__ token_ids, const float *__restrict__ counts, int n,
                                                              int n_tokens, float frequency_penalty, float presence_penalty, float repetition_penalty) {
  const int idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= n_tokens) return;
  const uint32_t token_id = token_ids[idx];
  if (token_id >= (uint32_t)n) return;
  const float count = counts[idx];
  if (count <= 0.0f) return;
  float value = logits[token_id];
  value -= fmaf(count, frequency_penalty, presence_penalty);  // `count * f + p` as nvcc contracts it (one rounding); this build has -ffp-contract=off, hence explicit
  if (repetition_penalty != 1.0f) value = value > 0.0f ? value / repetition_penalty : value * repetition_penalty;
  logits[token_id] = value;
}
__global__ void __launch_bounds__(NT) sparse_bias_kernel(float *__restrict__ logits, const uint32_t *__restrict__ token_ids, const float *__restrict__ biases, int n,
                                                         int n_tokens) {
  const int idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= n_tokens) return;
  const uint32_t token_id = token_ids[idx];
  if (token_id >= (uint32_t)n) return;
  logits[token_id] += biases[idx];  // token ids are unique in the caller's map (sampler.rs:1145-1160), as in the reference
}

// ---------------------------------------------------------------- the same pre-processing for ALL rows of a step in one launch: mrs_penalties_f32_batched (no reference
// counterpart: cuda_batch_sampling_plan gives up on a request with penalties, sampler.rs:617-631, and the single-row chain above costs a host hash map, uploads and up to
// three copy + update launch pairs per sequence and token, sampler.rs:1090-1169).  The launch takes the RAW token history of every row; counting and de-duplication happen here.
//   grid (chunks, rows), one workgroup per `chunk_size` logits of one row, the chunk in registers in load_chunk's assignment -- a logit is read, updated and stored by its
//   ONE owning thread, so x == dst is allowed;
//   the workgroup streams the row's whole context (L2-resident, re-read by every workgroup of the row: len * 4 bytes against chunk_size * 8 bytes of logits traffic) and
//   counts the tokens that fall in its chunk with integer LDS atomics: s_gen = occurrences at positions >= min(prompt_len, len), s_all = all occurrences;
//   the row's bias list is scanned the same way: s_bias[local] = 1 + the entry's index (ids are unique within a row: plain stores);
//   after one barrier: v = x; g > 0: v -= fmaf(g, f, p); s > 0 and rp != 1: v = v > 0 ? v / rp : v * rp; listed: v += bias -- the expressions of sparse_penalties_kernel and
//   sparse_bias_kernel, so dst equals the chain penalties(generated counts, f, p, 1) -> penalties(all counts, 0, 0, rp) -> bias bit for bit (sampler.rs:1111-1145).
// Integer atomics only, nothing crosses a workgroup: dst is a function of the row's inputs alone, whatever the launch, the batch row or the neighbours are.
struct PenArgs {
  const float *x;
  float *dst;
  const uint32_t *ctx_tokens;
  const int32_t *ctx_offsets, *prompt_lens;
  const float *frequency_penalties, *presence_penalties, *repetition_penalties;
  const uint32_t *bias_ids;
  const float *bias_values;
  const int32_t *bias_offsets;  // NULL: no bias in this launch
  int ncols, chunk_size;
};
constexpr int PEN_UNROLL = 4;  // context loads in flight per thread

__global__ void __launch_bounds__(NT) penalties_batched_kernel(PenArgs a) {
  __shared__ int s_gen[NT * MAXV], s_all[NT * MAXV], s_bias[NT * MAXV];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.y;
  const long long start = (long long)blockIdx.x * a.chunk_size, left = (long long)a.ncols - start;
  const int width = left <= 0 ? 0 : (left < a.chunk_size ? (int)left : a.chunk_size);
  const float *x = a.x + row * (size_t)a.ncols + start;
  float *dst = a.dst + row * (size_t)a.ncols + start;
  const int c0 = a.ctx_offsets[row], len = max(0, a.ctx_offsets[row + 1] - c0);
  const int b0 = a.bias_offsets ? a.bias_offsets[row] : 0, nbias = a.bias_offsets ? max(0, a.bias_offsets[row + 1] - b0) : 0;
  float v[MAXV];
  load_chunk(x, width, v);  // in flight while the context is counted
  if (len > 0 || nbias > 0) {  // uniform over the workgroup
    for (int i = tid; i < a.chunk_size; i += NT) {
      s_gen[i] = 0;
      s_all[i] = 0;
      if (nbias > 0) s_bias[i] = 0;
    }
    __syncthreads();
    const uint32_t *ctx = a.ctx_tokens + c0;
    const int gen_from = min(a.prompt_lens[row], len);  // positions from here on were generated
    for (int base = tid; base < len; base += PEN_UNROLL * NT) {
      uint32_t t[PEN_UNROLL];
#pragma unroll
      for (int j = 0; j < PEN_UNROLL; ++j) t[j] = base + j * NT < len ? ctx[base + j * NT] : 0xffffffffu;
#pragma unroll
      for (int j = 0; j < PEN_UNROLL; ++j) {
        const int pos = base + j * NT;
        const long long local = (long long)t[j] - start;  // ids >= ncols fall outside every chunk: ignored
        if (pos < len && local >= 0 && local < width) {
          atomicAdd(&s_all[local], 1);
          if (pos >= gen_from) atomicAdd(&s_gen[local], 1);
        }
      }
    }
    for (int e = tid; e < nbias; e += NT) {
      const long long local = (long long)a.bias_ids[b0 + e] - start;
      if (local >= 0 && local < width) s_bias[local] = e + 1;
    }
    __syncthreads();
    const float f = a.frequency_penalties[row], p = a.presence_penalties[row], rp = a.repetition_penalties[row];
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      const int local = tid + j * NT;
      if (local < width) {
        const int g = s_gen[local], s = s_all[local];
        float value = v[j];
        if (g > 0) value -= fmaf((float)g, f, p);  // one rounding, as sparse_penalties_kernel
        if (s > 0 && rp != 1.0f) value = value > 0.0f ? value / rp : value * rp;
        if (nbias > 0) {
          const int e = s_bias[local];
          if (e > 0) value += a.bias_values[b0 + e - 1];
        }
        v[j] = value;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    const int local = tid + j * NT;
    if (local < width) dst[local] = v[j];
  }
}

}  // namespace sampling
}  // namespace mrs

extern "C" void topk_large_f32(const float *input, float *block_values, uint32_t *block_indices, float *block_maxes, float *block_sums, float *values_out,
                               uint32_t *indices_out, float *softmax_info_out, int ncols, int k, int chunk_size, int nblocks, float inv_temperature,
                               int64_t stream) {
  mrs::sampling::run(input, nullptr, inv_temperature, block_values, block_indices, block_maxes, block_sums, nullptr, values_out, indices_out, softmax_info_out, 1,
                     ncols, k, chunk_size, nblocks, stream);
}
extern "C" void topk_large_f32_packed(const float *input, float *block_values, uint32_t *block_indices, float *block_maxes, float *block_sums, float *packed_out,
                                      int ncols, int k, int chunk_size, int nblocks, float inv_temperature, int64_t stream) {
  mrs::sampling::run(input, nullptr, inv_temperature, block_values, block_indices, block_maxes, block_sums, packed_out, nullptr, nullptr, nullptr, 1, ncols, k,
                     chunk_size, nblocks, stream);
}
extern "C" void topk_large_f32_packed_batched(const float *input, const float *inv_temperatures, float *block_values, uint32_t *block_indices, float *block_maxes,
                                              float *block_sums, float *packed_out, int nrows, int ncols, int k, int chunk_size, int nblocks, int64_t stream) {
  mrs::sampling::run(input, inv_temperatures, 0.0f, block_values, block_indices, block_maxes, block_sums, packed_out, nullptr, nullptr, nullptr, nrows, ncols, k,
                     chunk_size, nblocks, stream);
}
extern "C" void top1_large_f32_packed(const float *input, float *block_values, uint32_t *block_indices, float *packed_out, uint32_t *token_ids_out, int ncols,
                                      int chunk_size, int nblocks, int64_t stream) {
  mrs::sampling::run_top1(input, block_values, block_indices, packed_out, token_ids_out, 1, ncols, chunk_size, nblocks, stream);
}
extern "C" void top1_large_f32_packed_batched(const float *input, float *block_values, uint32_t *block_indices, float *packed_out, uint32_t *token_ids_out, int nrows,
                                              int ncols, int chunk_size, int nblocks, int64_t stream) {
  mrs::sampling::run_top1(input, block_values, block_indices, packed_out, token_ids_out, nrows, ncols, chunk_size, nblocks, stream);
}
extern "C" void categorical_large_f32_packed_batched(const float *input, const float *inv_temperatures, const float *uniforms, float *block_values, float *block_sums,
                                                     float *packed_out, int nrows, int ncols, int chunk_size, int nblocks, int64_t stream) {
  mrs::sampling::run_categorical(input, inv_temperatures, uniforms, block_values, block_sums, packed_out, nrows, ncols, chunk_size, nblocks, stream);
}
extern "C" void mrs_nucleus_large_f32_packed_batched(const float *input, const float *inv_temperatures, const float *uniforms, const float *top_ps, const float *min_ps,
                                                     float *block_values, float *block_sums, float *packed_out, int nrows, int ncols, int chunk_size, int nblocks,
                                                     int64_t stream) {
  mrs::sampling::run_nucleus(input, inv_temperatures, uniforms, top_ps, min_ps, block_values, block_sums, packed_out, nrows, ncols, chunk_size, nblocks, stream);
}
extern "C" size_t mrs_spec_verify_workspace_bytes(int total_rows, int nseq, int nblocks) { return mrs::sampling::spec_workspace_bytes(total_rows, nseq, nblocks); }
extern "C" void mrs_spec_verify_f32_batched(const float *target_logits, const float *draft_logits, const int32_t *draft_ids, const int32_t *seq_rows, const int32_t *modes,
                                            const float *inv_temperatures, const float *uniforms, void *workspace, size_t workspace_bytes, int32_t *n_accepted,
                                            int32_t *out_tokens, int nseq, int total_rows, int ncols, int chunk_size, int nblocks, int64_t stream) {
  mrs::sampling::run_spec_verify(target_logits, draft_logits, draft_ids, seq_rows, modes, inv_temperatures, uniforms, workspace, workspace_bytes, n_accepted, out_tokens,
                                 nseq, total_rows, ncols, chunk_size, nblocks, stream);
}
extern "C" void apply_sparse_penalties_f32(const void *x, void *dst, const uint32_t *token_ids, const float *counts, const int n, const int n_tokens,
                                           const float frequency_penalty, const float presence_penalty, const float repetition_penalty, int64_t stream) {
  using namespace mrs::sampling;
  if (n <= 0) return;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(copy_f32_kernel, dim3((n + NT * 4 - 1) / (NT * 4)), dim3(NT), 0, s, (const float *)x, (float *)dst, n);
  if (n_tokens <= 0) return;
  hipLaunchKernelGGL(sparse_penalties_kernel, dim3((n_tokens + NT - 1) / NT), dim3(NT), 0, s, (float *)dst, token_ids, counts, n, n_tokens, frequency_penalty,
                     presence_penalty, repetition_penalty);
}
extern "C" void apply_sparse_logits_bias_f32(const void *x, void *dst, const uint32_t *token_ids, const float *biases, const int n, const int n_tokens, int64_t stream) {
  using namespace mrs::sampling;
  if (n <= 0) return;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(copy_f32_kernel, dim3((n + NT * 4 - 1) / (NT * 4)), dim3(NT), 0, s, (const float *)x, (float *)dst, n);
  if (n_tokens <= 0) return;
  hipLaunchKernelGGL(sparse_bias_kernel, dim3((n_tokens + NT - 1) / NT), dim3(NT), 0, s, (float *)dst, token_ids, biases, n, n_tokens);
}
extern "C" void mrs_penalties_f32_batched(const float *x, float *dst, const uint32_t *ctx_tokens, const int32_t *ctx_offsets, const int32_t *prompt_lens,
                                          const float *frequency_penalties, const float *presence_penalties, const float *repetition_penalties,
                                          const uint32_t *bias_ids, const float *bias_values, const int32_t *bias_offsets, int nrows, int ncols, int chunk_size,
                                          int64_t stream) {
  using namespace mrs::sampling;
  if (nrows <= 0 || nrows > 65535 || ncols <= 0 || chunk_size < 1 || chunk_size > NT * MAXV) return;  // the rows are a grid dimension
  PenArgs a{x, dst, ctx_tokens, ctx_offsets, prompt_lens, frequency_penalties, presence_penalties, repetition_penalties, bias_ids, bias_values, bias_offsets, ncols,
            chunk_size};
  hipLaunchKernelGGL(penalties_batched_kernel, dim3((unsigned)(((long long)ncols + chunk_size - 1) / chunk_size), nrows), dim3(NT), 0, (hipStream_t)stream, a);
}

