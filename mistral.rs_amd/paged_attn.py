"""Host-side mirror of the `mistralrs-paged-attn` op surface
(mistralrs-paged-attn/src/cuda/backend/paged_attention.rs:453 `paged_attention`, :694 `reshape_and_cache`,
backend/gather_kv.rs `gather_kv_cache`, backend/cache.rs `copy_blocks`).

Same argument meaning, shape checks and v1/v2 selection rule as the reference; every call goes through the
C ABI of libmistralrspagedattention.so on the caller's current stream.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import torch

from . import _lib

_CODE = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}
_CACHE_CODE = {**_CODE, torch.uint8: 3}  # uint8 cache = fp8 E4M3 codes (cache_dtype 3): needs k_scale / v_scale (f32 scalars on the device)
if hasattr(torch, "float8_e4m3fn"):
    _CACHE_CODE[torch.float8_e4m3fn] = 3


def _scales(cache: torch.Tensor, k_scale, v_scale):
    """(k_scale ptr, v_scale ptr) for an fp8 cache, (None, None) otherwise; mirrors the Option<&Tensor> pair of the reference op."""
    if _CACHE_CODE.get(cache.dtype) != 3:
        return None, None
    if k_scale is None or v_scale is None:
        raise ValueError("an fp8 KV cache needs k_scale and v_scale")
    for t in (k_scale, v_scale):
        if t.dtype != torch.float32 or t.numel() != 1 or not t.is_cuda:
            raise ValueError("k_scale / v_scale must be single-element f32 GPU tensors")
    return k_scale.data_ptr(), v_scale.data_ptr()
_TAG = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
_HEAD_SIZES = (64, 80, 96, 112, 128, 192, 256, 512)
PARTITION_SIZE = 512
_vp, _i, _f, _u = C.c_void_p, C.c_int, C.c_float, C.c_uint32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


_ws: dict = {}


def _workspace(device, nbytes: int) -> torch.Tensor:
    key = (device.index, _stream())
    t = _ws.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = t
    return t


def _align_up(v: int, a: int) -> int:
    return (v + a - 1) // a * a


def kv_cache_shapes(num_blocks: int, num_kv_heads: int, head_size: int, block_size: int, dtype: torch.dtype):
    """K [nb, kvh, hd/x, bs, x], V [nb, kvh, hd, bs]  (mistralrs-core/src/paged_attention/cache_engine.rs:458-484)."""
    x = 16 // torch.empty((), dtype=dtype).element_size()
    return (num_blocks, num_kv_heads, head_size // x, block_size, x), (num_blocks, num_kv_heads, head_size, block_size)


def reshape_and_cache(key: torch.Tensor, value: torch.Tensor, key_cache: torch.Tensor, value_cache: torch.Tensor,
                      slot_mapping: torch.Tensor, k_scale: torch.Tensor | None = None, v_scale: torch.Tensor | None = None) -> None:
    """key/value [num_tokens, kv_heads, head_size] (row stride may exceed kv_heads*head_size);
    slot_mapping int64 [num_tokens]; negative slots are skipped."""
    if key.dtype not in _CODE:
        raise ValueError(f"dtype {key.dtype} is not supported")
    if key.dim() != 3 or value.shape != key.shape:
        raise ValueError(f"shape mismatch k {tuple(key.shape)} and v {tuple(value.shape)}")
    num_tokens, num_heads, head_size = key.shape
    nb, kvh, hs_x, block_size, x = key_cache.shape
    if kvh != num_heads or hs_x * x != head_size:
        raise ValueError(f"shape mismatch k {tuple(key.shape)} and key_cache {tuple(key_cache.shape)}")
    if tuple(value_cache.shape) != (nb, kvh, head_size, block_size):
        raise ValueError(f"shape mismatch key_cache {tuple(key_cache.shape)} and value_cache {tuple(value_cache.shape)}")
    if slot_mapping.dtype != torch.int64 or slot_mapping.numel() != num_tokens:
        raise ValueError(f"shape mismatch slot_mapping {tuple(slot_mapping.shape)}, expected {(num_tokens,)}")
    if key.stride(2) != 1 or key.stride(1) != head_size or value.stride(2) != 1 or value.stride(1) != head_size:
        raise ValueError("key/value must be contiguous within a token")
    fn = _lib.sym("paged_attn", "reshape_and_cache",
                  [_vp] * 5 + [_i] * 7 + [_vp, _u, _u, _vp, _vp])
    ks, vs = _scales(key_cache, k_scale, v_scale)
    fn(key.data_ptr(), value.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), slot_mapping.data_ptr(),
       num_tokens, num_heads, head_size, block_size, x, key.stride(0), value.stride(0), _stream(),
       _CODE[key.dtype], _CACHE_CODE[key_cache.dtype], ks, vs)


def paged_attention(q: torch.Tensor, key_cache: torch.Tensor, value_cache: torch.Tensor, block_tables: torch.Tensor,
                    context_lens: torch.Tensor, max_context_len: int, softmax_scale: float, softcapping: float = 1.0,
                    alibi_slopes: torch.Tensor | None = None, sinks: torch.Tensor | None = None,
                    force: str | None = None, k_scale: torch.Tensor | None = None, v_scale: torch.Tensor | None = None) -> torch.Tensor:
    """q [num_seqs, num_heads, head_size] (row stride free) -> out, same shape.  block_tables uint32/int32
    [num_seqs, max_blocks], context_lens uint32/int32 [num_seqs].  `force` in {None, 'v1', 'v2'} (tests)."""
    if q.dtype not in _CODE:
        raise ValueError(f"dtype {q.dtype} is not supported")
    if q.dim() != 3:
        raise ValueError("q must have rank 3")
    num_seqs, num_heads, head_size = q.shape
    if head_size not in _HEAD_SIZES:
        raise ValueError("`head_size` must be one of 64, 80, 96, 112, 128, 192, 256 or 512")
    if block_tables.dim() != 2 or block_tables.shape[0] != num_seqs:
        raise ValueError(f"shape mismatch block_tables {tuple(block_tables.shape)}, expected {(num_seqs, 'max_blocks')}")
    max_blocks = block_tables.shape[1]
    nb, kvh, hs_x, block_size, x = key_cache.shape
    if hs_x != head_size // x:
        raise ValueError(f"shape mismatch key_cache {tuple(key_cache.shape)}")
    if tuple(value_cache.shape) != (nb, kvh, head_size, block_size):
        raise ValueError(f"shape mismatch key_cache {tuple(key_cache.shape)} and value_cache {tuple(value_cache.shape)}")
    if tuple(context_lens.shape) != (num_seqs,):
        raise ValueError(f"shape mismatch context_lens {tuple(context_lens.shape)}, expected {(num_seqs,)}")
    if q.stride(2) != 1 or q.stride(1) != head_size:
        raise ValueError("q must be contiguous within a sequence row")
    eff_max = min(max_blocks * block_size, max_context_len)
    max_parts = (eff_max + PARTITION_SIZE - 1) // PARTITION_SIZE
    use_v1 = (max_parts == 1 or num_seqs * num_heads > 512) and PARTITION_SIZE % block_size == 0
    if force is not None:
        use_v1 = force == "v1"
    out = torch.empty(num_seqs, num_heads, head_size, dtype=q.dtype, device=q.device)
    al = alibi_slopes.data_ptr() if alibi_slopes is not None else None
    sk = sinks.data_ptr() if sinks is not None else None
    ks, vs = _scales(key_cache, k_scale, v_scale)
    fp8 = ks is not None
    if fp8 and block_size not in (16, 32):
        raise ValueError("an fp8 KV cache needs block_size 16 or 32")
    mixed = key_cache.dtype != q.dtype and not fp8
    if mixed and not (q.dtype == torch.float32 and key_cache.dtype == torch.bfloat16):
        raise ValueError(f"unsupported (query, cache) dtype pair ({q.dtype}, {key_cache.dtype})")
    common_tail = [_i, _f, _f, _vp, _vp] + [_i] * 9 + [_vp]
    if mixed:
        # MI355X-native entry: f32 activations over a bf16 cache
        fn = _lib.sym("paged_attn", "mrs_paged_attention_f32_bf16", [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp] + common_tail + [_vp])
        exp_sums = max_logits = tmp_out = None
        if not use_v1:
            ws = _paged_ws(q, num_seqs, num_heads, max_parts, head_size)
            tmp_out, exp_sums, max_logits = ws
        fn(0 if use_v1 else 1, out.data_ptr(), exp_sums, max_logits, tmp_out, q.data_ptr(), key_cache.data_ptr(),
           value_cache.data_ptr(), al, kvh, softmax_scale, softcapping, block_tables.data_ptr(), context_lens.data_ptr(),
           block_size, eff_max, num_seqs, num_heads, head_size, max_blocks, q.stride(0), key_cache.stride(0),
           key_cache.stride(1), _stream(), sk)
        return out
    tail = common_tail + [_u, _vp, _vp, _vp]
    if use_v1:
        fn = _lib.sym("paged_attn", f"paged_attention_v1_{_TAG[q.dtype]}", [_vp] * 5 + tail)
        fn(out.data_ptr(), q.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), al, kvh, softmax_scale, softcapping,
           block_tables.data_ptr(), context_lens.data_ptr(), block_size, eff_max, num_seqs, num_heads, head_size,
           max_blocks, q.stride(0), key_cache.stride(0), key_cache.stride(1), _stream(), _CACHE_CODE[key_cache.dtype], ks, vs, sk)
    else:
        tmp_out, exp_sums, max_logits = _paged_ws(q, num_seqs, num_heads, max_parts, head_size)
        fn = _lib.sym("paged_attn", f"paged_attention_v2_{_TAG[q.dtype]}", [_vp] * 8 + tail)
        fn(out.data_ptr(), exp_sums, max_logits, tmp_out, q.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), al, kvh,
           softmax_scale, softcapping, block_tables.data_ptr(), context_lens.data_ptr(), block_size, eff_max, num_seqs,
           num_heads, head_size, max_blocks, q.stride(0), key_cache.stride(0), key_cache.stride(1), _stream(),
           _CACHE_CODE[key_cache.dtype], ks, vs, sk)
    return out


def _paged_ws(q, num_seqs, num_heads, max_parts, head_size):
    """v2 workspace carve-up, as backend/paged_attention.rs:353-365."""
    tmp_bytes = num_seqs * num_heads * max_parts * head_size * q.element_size()
    es_bytes = num_seqs * num_heads * max_parts * 4
    es_off = _align_up(tmp_bytes, 16)
    ml_off = _align_up(es_off + es_bytes, 16)
    ws = _workspace(q.device, ml_off + es_bytes)
    base = ws.data_ptr()
    return base, base + es_off, base + ml_off


def gather_kv_cache(key_cache: torch.Tensor, value_cache: torch.Tensor, block_table: torch.Tensor,
                    cu_seq_lens: torch.Tensor, out_dtype: torch.dtype, k_scale: torch.Tensor | None = None,
                    v_scale: torch.Tensor | None = None):
    """paged -> dense K/V [num_tokens, kv_heads, head_size]; cu_seq_lens int32 [num_seqs + 1]."""
    nb, kvh, hs_x, block_size, x = key_cache.shape
    head_size = hs_x * x
    num_seqs = cu_seq_lens.numel() - 1
    num_tokens = int(cu_seq_lens[-1].item())
    k_out = torch.empty(num_tokens, kvh, head_size, dtype=out_dtype, device=key_cache.device)
    v_out = torch.empty_like(k_out)
    fn = _lib.sym("paged_attn", "gather_kv_cache", [_vp] * 8 + [_i] * 7 + [_vp, _u, _u])
    ks, vs = _scales(key_cache, k_scale, v_scale)
    fn(key_cache.data_ptr(), value_cache.data_ptr(), k_out.data_ptr(), v_out.data_ptr(), ks, vs,
       block_table.data_ptr(), cu_seq_lens.data_ptr(), num_tokens, num_seqs, block_size, block_table.stride(0), kvh,
       head_size, x, _stream(), _CODE[out_dtype], _CACHE_CODE[key_cache.dtype])
    return k_out, v_out


def update_kv_scales(key: torch.Tensor, value: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor) -> None:
    """k_scale = max(k_scale, absmax(key) / 240), same for v, in place (backend/scale_update.rs:81-105, update_kvscales.cu)."""
    if key.dtype not in _CODE or value.dtype != key.dtype or key.numel() != value.numel():
        raise ValueError("update_kv_scales: key / value must share dtype (f16 / bf16 / f32) and element count")
    if not (key.is_contiguous() and value.is_contiguous()):
        raise ValueError("update_kv_scales: key / value must be contiguous")
    for t in (k_scale, v_scale):
        if t.dtype != torch.float32 or t.numel() != 1:
            raise ValueError("k_scale / v_scale must be single-element f32 tensors")
    fn = _lib.sym("paged_attn", f"update_kv_scales_{_TAG[key.dtype]}", [_vp, _vp, C.c_long, _vp, _vp, C.c_int64])
    fn(key.data_ptr(), value.data_ptr(), key.numel(), k_scale.data_ptr(), v_scale.data_ptr(), _stream())


def copy_blocks(key_caches: list, value_caches: list, block_mapping: dict) -> None:
    """For every layer copy block src -> each dst (copy-on-write).  Mirrors backend/cache.rs `copy_blocks`."""
    if not key_caches or not block_mapping:
        return
    dev = key_caches[0].device
    pairs = [(s, d) for s, ds in block_mapping.items() for d in (ds if isinstance(ds, (list, tuple)) else [ds])]
    kp = torch.tensor([t.data_ptr() for t in key_caches], dtype=torch.int64, device=dev)
    vp = torch.tensor([t.data_ptr() for t in value_caches], dtype=torch.int64, device=dev)
    bm = torch.tensor(pairs, dtype=torch.int64, device=dev).reshape(-1)
    tag = {2: "bf16" if key_caches[0].dtype == torch.bfloat16 else "f16", 4: "f32", 1: "u8"}[key_caches[0].element_size()]
    fn = _lib.sym("paged_attn", f"copy_blocks_{tag}", [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64])
    fn(kp.data_ptr(), vp.data_ptr(), bm.data_ptr(), len(key_caches), len(pairs), key_caches[0][0].numel(),
       value_caches[0][0].numel(), _stream())
    torch.cuda.current_stream().synchronize()  # keep kp/vp/bm alive until the copy ran


def decode_attention_q8_1(q: torch.Tensor, key_cache: torch.Tensor, value_cache: torch.Tensor, block_tables: torch.Tensor,
                          context_lens: torch.Tensor, max_context_len: int, softmax_scale: float) -> tuple[torch.Tensor, int]:
    """MI355X-native decode attention of the fused path (mrs_decode_attention_q8_1_f32_bf16): f32 q [seqs, heads, hd]
    over a bf16 paged cache -> Q8_1 blocks [seqs, stride_blocks * 36] uint8 (o_proj's activation format).
    Returns (blocks, stride_blocks).  Raises ValueError for shapes the kernel refuses."""
    if q.dtype != torch.float32 or key_cache.dtype != torch.bfloat16 or q.dim() != 3:
        raise ValueError("decode_attention_q8_1: f32 query [seqs, heads, hd] over a bf16 cache")
    num_seqs, num_heads, head_size = q.shape
    nb, kvh, hs_x, block_size, x = key_cache.shape
    max_blocks = block_tables.shape[1]
    eff_max = min(max_blocks * block_size, max_context_len)
    L = _lib.load("paged_attn")
    L.mrs_decode_attention_max_splits.argtypes = [_i]
    splits = L.mrs_decode_attention_max_splits(eff_max)
    nq = num_heads * head_size
    stride_blocks = _align_up(nq, 512) // 32
    y = torch.zeros(num_seqs, stride_blocks * 36, dtype=torch.uint8, device=q.device)
    tmp = torch.empty(num_seqs * num_heads * splits * head_size, dtype=torch.float32, device=q.device)
    es = torch.empty(num_seqs * num_heads * splits, dtype=torch.float32, device=q.device)
    ml = torch.empty_like(es)
    fn = _lib.sym("paged_attn", "mrs_decode_attention_q8_1_f32_bf16",
                  [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp] + [_i] * 9 + [_vp], _i)
    rc = fn(y.data_ptr(), stride_blocks, es.data_ptr(), ml.data_ptr(), tmp.data_ptr(), q.data_ptr(), key_cache.data_ptr(),
            value_cache.data_ptr(), kvh, softmax_scale, block_tables.data_ptr(), context_lens.data_ptr(), block_size, eff_max,
            num_seqs, num_heads, head_size, max_blocks, q.stride(0), key_cache.stride(0), key_cache.stride(1), _stream())
    if rc != 0:
        raise ValueError("decode_attention_q8_1: unsupported shape (block_size 32, head_size 64/128)")
    return y, stride_blocks


_SINK_HEAD_DIMS = (64, 80, 96, 112, 128, 192, 256)


def _sinks_checks(name: str, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, sinks, kv_rank: int):
    """Shared checks of the two ops below (backend/flash_attn_sinks.rs:26-58,184-196); returns the sinks pointer or None."""
    if q.dtype not in _CODE:
        raise ValueError(f"{name}: only f32 / f16 / bf16 are supported, got {q.dtype}")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"{name}: q, k and v must share one dtype")
    if q.dim() != 4 or k.dim() != kv_rank or v.shape != k.shape:
        raise ValueError(f"{name}: shape mismatch q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise ValueError(f"{name}: q, k and v must be GPU tensors")
    if not (q.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
        raise ValueError(f"{name}: q, k and v must be contiguous")
    num_heads, head_dim = q.shape[1], q.shape[3]
    if head_dim not in _SINK_HEAD_DIMS:
        raise ValueError(f"{name}: head_dim must be one of 64, 80, 96, 112, 128, 192, 256, got {head_dim}")
    num_kv_heads = k.shape[-2] if kv_rank == 3 else k.shape[1]
    if k.shape[-1] != head_dim or num_kv_heads == 0 or num_heads % num_kv_heads:
        raise ValueError(f"{name}: k {tuple(k.shape)} does not match q {tuple(q.shape)}")
    if sinks is None:
        return None
    if sinks.dtype != torch.float32 or tuple(sinks.shape) != (num_heads,) or not sinks.is_cuda or not sinks.is_contiguous():
        raise ValueError(f"{name}: sinks must be a contiguous f32 GPU tensor [{num_heads}]")
    return sinks.data_ptr()


def flash_attn_sinks(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, sinks: torch.Tensor | None, softmax_scale: float,
                     window_size: int) -> torch.Tensor:
    """Causal prompt attention with per-head sinks (backend/flash_attn_sinks.rs:320 `flash_attn_sinks`): q [B, H, q_len, D],
    k / v [B, Hkv, kv_len, D], sinks f32 [H] or None, window_size 0 = no window -> [B, H, q_len, D].  The mask is aligned to the bottom right
    (row r sees keys up to r + kv_len - q_len); a sink adds exp(sink) to the softmax denominator and no value."""
    sk = _sinks_checks("flash_attn_sinks", q, k, v, sinks, 4)
    batch, num_heads, q_len, head_dim = q.shape
    if k.shape[0] != batch:
        raise ValueError(f"flash_attn_sinks: k {tuple(k.shape)} does not match q {tuple(q.shape)}")
    if window_size < 0:
        raise ValueError("flash_attn_sinks: window_size must be >= 0")
    out = torch.empty_like(q)
    fn = _lib.sym("paged_attn", f"flash_attn_sinks_{_TAG[q.dtype]}", [_vp] * 5 + [_f] + [_i] * 7 + [_vp])
    fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), sk, softmax_scale, batch, q_len, k.shape[2], num_heads, k.shape[1], head_dim,
       window_size, _stream())
    return out


def flash_attn_sinks_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, sinks: torch.Tensor | None, cu_seqlens_q: torch.Tensor,
                            cu_seqlens_k: torch.Tensor, softmax_scale: float, window_size: int) -> torch.Tensor:
    """Variable-length form (backend/flash_attn_sinks.rs:360 `flash_attn_sinks_varlen`): q padded [B, H, max_q_len, D], k / v packed
    [total_kv, Hkv, D], cu_seqlens_q / cu_seqlens_k uint32 [B + 1] -> [B, H, max_q_len, D] with the padding rows zero."""
    sk = _sinks_checks("flash_attn_sinks_varlen", q, k, v, sinks, 3)
    batch, num_heads, max_q_len, head_dim = q.shape
    for name, t in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if t.dtype != torch.uint32 or tuple(t.shape) != (batch + 1,) or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"flash_attn_sinks_varlen: {name} must be a contiguous uint32 GPU tensor [{batch + 1}]")
    if window_size < 0:
        raise ValueError("flash_attn_sinks_varlen: window_size must be >= 0")
    out = torch.zeros_like(q)
    fn = _lib.sym("paged_attn", f"flash_attn_sinks_varlen_{_TAG[q.dtype]}", [_vp] * 7 + [_f] + [_i] * 6 + [_vp])
    fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), sk, cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), softmax_scale, batch,
       max_q_len, num_heads, k.shape[1], head_dim, window_size, _stream())
    return out


_MLA_DIMS = (512, 64)  # kv_lora_rank, rotary head dim: what the decode kernel is built for (backend/mla.rs:262)
_MLA_CUS = 256         # compute units of the MI355X, one decode workgroup each


def _mla_caches(name: str, ckv_cache: torch.Tensor, kpe_cache: torch.Tensor, dtype):
    """Shared cache checks of the three MLA ops (backend/mla.rs:25-31,66-84,659-663); returns (block_size, kv_lora_rank, kpe_head_dim)."""
    if dtype not in _CODE:
        raise ValueError(f"{name}: only f16 / bf16 / f32 are supported, got {dtype}")
    if ckv_cache.dtype != dtype or kpe_cache.dtype != dtype:
        raise ValueError(f"{name}: cache dtypes {ckv_cache.dtype} / {kpe_cache.dtype} do not match {dtype}")
    if ckv_cache.dim() != 3 or kpe_cache.dim() != 3 or ckv_cache.shape[:2] != kpe_cache.shape[:2]:
        raise ValueError(f"{name}: block shape mismatch ckv_cache {tuple(ckv_cache.shape)} and kpe_cache {tuple(kpe_cache.shape)}")
    if not (ckv_cache.is_cuda and kpe_cache.is_cuda and ckv_cache.is_contiguous() and kpe_cache.is_contiguous()):
        raise ValueError(f"{name}: the caches must be contiguous GPU tensors")
    return ckv_cache.shape[1], ckv_cache.shape[2], kpe_cache.shape[2]


def _mla_meta(name: str, what: str, t: torch.Tensor, numel: int | None = None) -> torch.Tensor:
    if t.dtype != torch.int32 or t.dim() != 1 or not t.is_cuda or (numel is not None and t.numel() != numel):
        raise ValueError(f"{name}: {what} must be an int32 GPU vector" + ("" if numel is None else f" of length {numel}") + f", got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def concat_and_cache_mla(ckv: torch.Tensor, k_pe: torch.Tensor, ckv_cache: torch.Tensor, kpe_cache: torch.Tensor, slot_mapping: torch.Tensor) -> None:
    """Write one latent row and one rotary row per token into the paged MLA cache (backend/mla.rs:10 `concat_and_cache_mla`): ckv [T, kv_lora_rank],
    k_pe [T, kpe_head_dim] (row strides may exceed the row), caches [num_blocks, block_size, rank / dim], slot_mapping int64 [T]; negative slots are skipped."""
    name = "concat_and_cache_mla"
    if k_pe.dtype != ckv.dtype:
        raise ValueError(f"{name}: ckv and k_pe must share one dtype, got {ckv.dtype} and {k_pe.dtype}")
    block_size, rank, pe_dim = _mla_caches(name, ckv_cache, kpe_cache, ckv.dtype)
    if ckv.dim() != 2 or k_pe.dim() != 2 or ckv.shape[0] != k_pe.shape[0] or ckv.shape[1] != rank or k_pe.shape[1] != pe_dim:
        raise ValueError(f"{name}: shape mismatch ckv {tuple(ckv.shape)}, k_pe {tuple(k_pe.shape)}, caches {tuple(ckv_cache.shape)} / {tuple(kpe_cache.shape)}")
    if not (ckv.is_cuda and k_pe.is_cuda) or ckv.stride(1) != 1 or k_pe.stride(1) != 1:
        raise ValueError(f"{name}: ckv and k_pe must be GPU tensors with contiguous rows")
    num_tokens = ckv.shape[0]
    if slot_mapping.dtype != torch.int64 or slot_mapping.dim() != 1 or slot_mapping.numel() != num_tokens or not slot_mapping.is_cuda:
        raise ValueError(f"{name}: slot_mapping must be an int64 GPU vector of length {num_tokens}")
    fn = _lib.sym("paged_attn", "concat_and_cache_mla", [_vp] * 5 + [_i] * 6 + [_vp, _u])
    fn(ckv.data_ptr(), k_pe.data_ptr(), ckv_cache.data_ptr(), kpe_cache.data_ptr(), slot_mapping.contiguous().data_ptr(), num_tokens, rank, pe_dim,
       block_size, ckv.stride(0), k_pe.stride(0), _stream(), _CODE[ckv.dtype])


def gather_mla_cache(ckv_cache: torch.Tensor, kpe_cache: torch.Tensor, block_table: torch.Tensor, cu_seq_lens: torch.Tensor,
                     token_to_seq: torch.Tensor):
    """Paged MLA cache -> dense (ckv [T, kv_lora_rank], kpe [T, kpe_head_dim]) (backend/mla.rs:643 `gather_mla_cache`): token i is position
    i - cu_seq_lens[s] of sequence s = token_to_seq[i]; block_table int32 [seqs, max_blocks], cu_seq_lens int32 [seqs + 1], token_to_seq int32 [T]."""
    name = "gather_mla_cache"
    block_size, rank, pe_dim = _mla_caches(name, ckv_cache, kpe_cache, ckv_cache.dtype)
    if block_table.dtype != torch.int32 or block_table.dim() != 2 or not block_table.is_cuda:
        raise ValueError(f"{name}: block_table must be an int32 GPU matrix, got {block_table.dtype} {tuple(block_table.shape)}")
    block_table = block_table.contiguous()
    cu_seq_lens = _mla_meta(name, "cu_seq_lens", cu_seq_lens, block_table.shape[0] + 1)
    token_to_seq = _mla_meta(name, "token_to_seq", token_to_seq)
    num_tokens = token_to_seq.numel()
    ckv = torch.zeros(num_tokens, rank, dtype=ckv_cache.dtype, device=ckv_cache.device)
    kpe = torch.zeros(num_tokens, pe_dim, dtype=ckv_cache.dtype, device=ckv_cache.device)
    fn = _lib.sym("paged_attn", "gather_mla_cache", [_vp] * 7 + [_i] * 5 + [_vp, _u])
    fn(ckv_cache.data_ptr(), kpe_cache.data_ptr(), ckv.data_ptr(), kpe.data_ptr(), block_table.data_ptr(), cu_seq_lens.data_ptr(),
       token_to_seq.data_ptr(), num_tokens, block_size, block_table.stride(0), rank, pe_dim, _stream(), _CODE[ckv_cache.dtype])
    return ckv, kpe


def mla_decode_splits(batch: int, num_heads: int, max_kv_len: int) -> int:
    """KV splits for `flashinfer_mla_decode` from host-known quantities: enough workgroups (batch x head blocks x splits) to cover the compute units,
    but no split shorter than 16 tiles of 32 keys for a 64-head block, 8 for a 32-head one: a split's f32 partial (2 KiB per head, written and read
    back) then stays under half of the 36 KiB per tile that it reads."""
    groups = max(1, batch * (-(-num_heads // 64)))
    tiles = -(-max(max_kv_len, 1) // 32)
    return max(1, min(_MLA_CUS // groups, tiles // (16 if num_heads > 32 else 8), 128))


def flashinfer_mla_decode(q_nope: torch.Tensor, q_pe: torch.Tensor, ckv_cache: torch.Tensor, kpe_cache: torch.Tensor, paged_kv_indptr: torch.Tensor,
                          paged_kv_indices: torch.Tensor, paged_kv_last_page_len: torch.Tensor, sm_scale: float, *, num_splits: int | None = None,
                          max_kv_len: int | None = None) -> torch.Tensor:
    """MLA decode over the paged latent cache (backend/mla.rs:227 `flashinfer_mla_decode`): q_nope [batch, heads, 512], q_pe [batch, heads, 64] (rotated),
    caches [num_blocks, page_size, 512 / 64] with page_size 16 or 32, f16 or bf16; request b owns pages paged_kv_indices[indptr[b] : indptr[b + 1]] with
    paged_kv_last_page_len[b] keys in the last one -> [batch, heads, 512]; a request without keys gets zeros.  num_splits None picks the split count
    from batch, head blocks and max_kv_len (default: paged_kv_indices.numel() * page_size, an upper bound); nothing is read back from the device."""
    name = "flashinfer_mla_decode"
    if q_pe.dtype != q_nope.dtype:
        raise ValueError(f"{name}: q_nope and q_pe must share one dtype, got {q_nope.dtype} and {q_pe.dtype}")
    if q_nope.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{name}: only f16 / bf16 are supported, got {q_nope.dtype}")
    page_size, rank, pe_dim = _mla_caches(name, ckv_cache, kpe_cache, q_nope.dtype)
    if q_nope.dim() != 3 or q_pe.dim() != 3 or q_nope.shape[:2] != q_pe.shape[:2]:
        raise ValueError(f"{name}: shape mismatch q_nope {tuple(q_nope.shape)} and q_pe {tuple(q_pe.shape)}")
    batch, num_heads = q_nope.shape[:2]
    if (q_nope.shape[2], q_pe.shape[2]) != _MLA_DIMS or (rank, pe_dim) != _MLA_DIMS:
        raise ValueError(f"{name}: head dims must be 512 / 64, got q {q_nope.shape[2]} / {q_pe.shape[2]}, caches {rank} / {pe_dim}")
    if page_size not in (16, 32):
        raise ValueError(f"{name}: page size must be 16 or 32, got {page_size}")
    if num_heads < 1 or not (q_nope.is_cuda and q_pe.is_cuda and q_nope.is_contiguous() and q_pe.is_contiguous()):
        raise ValueError(f"{name}: q_nope and q_pe must be contiguous GPU tensors with at least one head")
    indptr = _mla_meta(name, "paged_kv_indptr", paged_kv_indptr, batch + 1)
    last = _mla_meta(name, "paged_kv_last_page_len", paged_kv_last_page_len, batch)
    indices = _mla_meta(name, "paged_kv_indices", paged_kv_indices)
    if num_splits is None:
        num_splits = mla_decode_splits(batch, num_heads, indices.numel() * page_size if max_kv_len is None else max_kv_len)
    if num_splits < 1:
        raise ValueError(f"{name}: num_splits must be >= 1")
    out = torch.empty_like(q_nope)
    nbytes = _lib.sym("paged_attn", "mla_decode_workspace_bytes", [_i] * 3, C.c_size_t)(batch, num_heads, num_splits)
    ws = _workspace(q_nope.device, nbytes) if nbytes else None
    fn = _lib.sym("paged_attn", "launch_mla_decode", [_vp] * 8 + [_i] * 3 + [_f, _i, _vp, C.c_size_t, _u, _vp], _i)
    rc = fn(q_nope.data_ptr(), q_pe.data_ptr(), ckv_cache.data_ptr(), kpe_cache.data_ptr(), indptr.data_ptr(), indices.data_ptr(), last.data_ptr(),
            out.data_ptr(), batch, num_heads, page_size, sm_scale, num_splits, None if ws is None else ws.data_ptr(), nbytes, _CODE[q_nope.dtype],
            _stream())
    if rc != 0:
        raise RuntimeError(f"{name}: launch_mla_decode returned {rc}")
    return out


# ---------------------------------------------------------------------------------- FlashInfer-layout (HND) cache, CSR requests, tile plan
_FI_HEAD_SIZES = (64, 128, 256)  # what the decode kernel is built for; 512 is refused (deviations)
_FI_CUS = 256                    # compute units of the MI355X


class FlashInferDecodePlan(NamedTuple):
    """The split-KV tile plan of `flashinfer_decode`: int32 [padded], int32 [padded], int32 [batch + 1], int32 [1], uint8 [padded]."""
    request_indices: torch.Tensor
    kv_tile_indices: torch.Tensor
    o_indptr: torch.Tensor
    kv_chunk_size: torch.Tensor
    block_valid_mask: torch.Tensor


def flashinfer_cache_shape(num_blocks: int, num_kv_heads: int, head_size: int, block_size: int):
    """K and V caches of the FlashInfer path share one shape, [num_pages, kv_heads, page_size, head_size] (HND): a key row is head_size contiguous
    elements.  Neither cache can be read by `paged_attention` (x-packed K, transposed V: `kv_cache_shapes`), nor the reverse."""
    return (num_blocks, num_kv_heads, block_size, head_size)


def _fi_cache(name: str, dtype, key_cache: torch.Tensor, value_cache: torch.Tensor, k_scale: float, v_scale: float):
    """validate_cache_dtype / validate_cache_scales and the cache shape checks of backend/flashinfer.rs:35-62,109-112; returns the cache dtype code."""
    if dtype not in _CODE:
        raise ValueError(f"{name} only supports f16, bf16, f32 (got {dtype})")
    if key_cache.dtype not in _CACHE_CODE or value_cache.dtype != key_cache.dtype:
        raise ValueError(f"{name} expects matching cache dtypes out of f16, bf16, f32, f8e4m3 (got {key_cache.dtype}, {value_cache.dtype})")
    code = _CACHE_CODE[key_cache.dtype]
    if code != 3 and key_cache.dtype != dtype:
        raise ValueError(f"{name} requires matching activation/cache dtypes or an f8e4m3 cache, got activation={dtype}, cache={key_cache.dtype}")
    if not (math.isfinite(k_scale) and k_scale > 0.0 and math.isfinite(v_scale) and v_scale > 0.0):
        raise ValueError(f"{name} requires finite positive K/V cache scales, got k={k_scale} v={v_scale}")
    if code != 3 and (k_scale != 1.0 or v_scale != 1.0):
        raise ValueError(f"{name} only accepts non-unit cache scales for f8e4m3 caches, got cache={key_cache.dtype} k={k_scale} v={v_scale}")
    if key_cache.dim() != 4 or value_cache.shape != key_cache.shape:
        raise ValueError(f"{name} cache shape mismatch: {tuple(key_cache.shape)} and {tuple(value_cache.shape)}")
    if not (key_cache.is_cuda and value_cache.is_cuda and key_cache.is_contiguous() and value_cache.is_contiguous()):
        raise ValueError(f"{name}: the caches must be contiguous GPU tensors")
    return code


def reshape_and_cache_flashinfer(key: torch.Tensor, value: torch.Tensor, key_cache: torch.Tensor, value_cache: torch.Tensor, slot_mapping: torch.Tensor,
                                 k_scale: float = 1.0, v_scale: float = 1.0) -> None:
    """Scatter key / value [T, kv_heads, head_size] (row stride free) into the HND caches (backend/flashinfer.rs:71 `reshape_and_cache_flashinfer`):
    token i goes to slot slot_mapping[i] = page * page_size + row (int64; negative slots are skipped).  An E4M3 cache stores value / scale."""
    name = "reshape_and_cache_flashinfer"
    if value.dtype != key.dtype:
        raise ValueError(f"{name} expects matching K/V dtypes, got key={key.dtype}, value={value.dtype}")
    code = _fi_cache(name, key.dtype, key_cache, value_cache, k_scale, v_scale)
    if slot_mapping.dtype != torch.int64:
        raise ValueError(f"{name} expects i64 slot_mapping")
    if key.dim() != 3 or value.shape != key.shape:
        raise ValueError(f"{name} key/value shape mismatch: {tuple(key.shape)} vs {tuple(value.shape)}")
    num_tokens, num_heads, head_size = key.shape
    for t in (key, value):
        if not t.is_cuda or t.stride(2) != 1 or t.stride(1) != head_size:
            raise ValueError(f"{name}: key / value must be GPU tensors, contiguous within a token")
    _, cache_heads, block_size, cache_head_size = key_cache.shape
    if cache_heads != num_heads or cache_head_size != head_size:
        raise ValueError(f"{name} cache shape {tuple(key_cache.shape)} incompatible with key {tuple(key.shape)}")
    if slot_mapping.dim() != 1 or slot_mapping.numel() != num_tokens or not slot_mapping.is_cuda:
        raise ValueError(f"{name} slot_mapping length mismatch: expected {num_tokens}, got {tuple(slot_mapping.shape)}")
    fn = _lib.sym("paged_attn", "reshape_and_cache_flashinfer", [_vp] * 5 + [_i] * 6 + [_f, _f, _u, _u, _vp])
    fn(key.data_ptr(), value.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), slot_mapping.contiguous().data_ptr(), num_tokens, num_heads,
       head_size, block_size, key.stride(0), value.stride(0), k_scale, v_scale, _CODE[key.dtype], code, _stream())


def gather_kv_cache_flashinfer(key_cache: torch.Tensor, value_cache: torch.Tensor, block_table: torch.Tensor, cu_seq_lens: torch.Tensor,
                               out_dtype: torch.dtype, k_scale: float = 1.0, v_scale: float = 1.0):
    """HND pages -> dense (K, V) [num_tokens, kv_heads, head_size] (backend/flashinfer.rs:550 `gather_kv_cache_flashinfer`); block_table int32
    [seqs, max_blocks], cu_seq_lens int32 [seqs + 1] (its last entry is read back: it sizes the outputs).  E4M3 pages come back times the scale."""
    name = "gather_kv_cache_flashinfer"
    code = _fi_cache(name, out_dtype, key_cache, value_cache, k_scale, v_scale)
    if block_table.dtype != torch.int32 or cu_seq_lens.dtype != torch.int32 or block_table.dim() != 2 or cu_seq_lens.dim() != 1:
        raise ValueError(f"{name} expects i32 metadata: block_table [seqs, max_blocks], cu_seq_lens [seqs + 1]")
    num_seqs = cu_seq_lens.numel() - 1
    if block_table.shape[0] != num_seqs or not (block_table.is_cuda and cu_seq_lens.is_cuda):
        raise ValueError(f"{name}: block_table {tuple(block_table.shape)} does not match cu_seq_lens {tuple(cu_seq_lens.shape)}")
    block_table, cu_seq_lens = block_table.contiguous(), cu_seq_lens.contiguous()
    _, kvh, block_size, head_size = key_cache.shape
    num_tokens = int(cu_seq_lens[-1].item())
    k_out = torch.empty(num_tokens, kvh, head_size, dtype=out_dtype, device=key_cache.device)
    v_out = torch.empty_like(k_out)
    if num_tokens:
        fn = _lib.sym("paged_attn", "gather_kv_cache_flashinfer", [_vp] * 6 + [_i] * 6 + [_u, _u, _f, _f, _vp])
        fn(key_cache.data_ptr(), value_cache.data_ptr(), k_out.data_ptr(), v_out.data_ptr(), block_table.data_ptr(), cu_seq_lens.data_ptr(), num_tokens,
           num_seqs, block_size, block_table.stride(0), kvh, head_size, _CODE[out_dtype], code, k_scale, v_scale, _stream())
    return k_out, v_out


def flashinfer_decode_plan(context_lens, block_size: int, split_pages: int | None = None, padded_tiles_len: int | None = None,
                           device=None) -> FlashInferDecodePlan:
    """Host-side twin of `make_paged_kv_decode_tensors` (mistralrs-core/src/flashinfer/metadata.rs:150-216): request b gets
    ceil(max(pages_b, 1) / split_pages) plan tiles (one with split_pages None), each split_pages * block_size keys (block_size with None, as there);
    o_indptr counts them.  The lists are padded with zeros, mask 0, to padded_tiles_len (default: no padding, at least one entry) so that a captured
    graph replays any plan of that size; more tiles than that is an error."""
    chunk_pages = max(split_pages, 1) if split_pages is not None else None
    req, tile, o_indptr = [], [], [0]
    for b, n in enumerate(context_lens):
        pages = max(-(-int(n) // block_size), 1)
        chunks = 1 if chunk_pages is None else -(-pages // chunk_pages)
        req += [b] * chunks
        tile += list(range(chunks))
        o_indptr.append(len(req))
    valid = len(req)
    if padded_tiles_len is None:
        padded_tiles_len = max(valid, 1)
    if valid > padded_tiles_len:
        raise ValueError(f"paged kv decode tiles exceed padded length: tiles={valid} padded={padded_tiles_len}")
    pad = [0] * (padded_tiles_len - valid)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=device)
    return FlashInferDecodePlan(i32(req + pad), i32(tile + pad), i32(o_indptr), i32([(split_pages or 1) * block_size]),
                                torch.tensor([1] * valid + pad, dtype=torch.uint8, device=device))


def flashinfer_decode_split_pages(batch: int, num_kv_heads: int, max_kv_len: int, page_size: int) -> int:
    """`split_pages` for `flashinfer_decode_plan` from host-known numbers.  The grid is (plan tiles, kv_heads) and a workgroup streams its keys with four
    waves at one to three workgroups per compute unit, so the plan should offer about two workgroups per compute unit: chunks = 2 * 256 / (batch *
    kv_heads).  A chunk is not made shorter than 256 keys: below that a wave has fewer than two 32-key tiles and nothing to overlap its loads with,
    while the f32 partial a chunk writes (and the merge reads back) is, at G * head_size * 4 bytes against 256 * head_size * 4 bytes of bf16 K and V,
    still under G / 256 of what the chunk reads.  One chunk (the return value covers max_kv_len) means the plan has one tile per request: the caller
    may then pass partition=False and save the merge launch."""
    pages = max(-(-max(max_kv_len, 1) // page_size), 1)
    chunks = max(1, min(-(-2 * _FI_CUS // max(batch * num_kv_heads, 1)), pages * page_size // 256))
    return -(-pages // chunks)


def flashinfer_decode(q: torch.Tensor, key_cache: torch.Tensor, value_cache: torch.Tensor, paged_kv_indptr: torch.Tensor, paged_kv_indices: torch.Tensor,
                      paged_kv_last_page_len: torch.Tensor, plan, sm_scale: float, *, window_left: int | None = None,
                      logits_soft_cap: float | None = None, k_scale: float = 1.0, v_scale: float = 1.0, partition: bool = True) -> torch.Tensor:
    """GQA decode over the HND paged cache (backend/flashinfer.rs:241 `flashinfer_decode`): q [batch, heads, head_size] (strides of the first two dims
    free), f16 / bf16, caches of the same dtype or E4M3; request b owns pages paged_kv_indices[indptr[b] : indptr[b + 1]] with
    paged_kv_last_page_len[b] keys in the last one; `plan` is the five tensors of `flashinfer_decode_plan` on the GPU -> [batch, heads, head_size];
    a request without a visible key gets zeros.  window_left: key i is visible iff i + 1 + window_left >= kv_len; logits_soft_cap: s -> cap *
    tanh(s / cap).  partition=False passes no scratch (tmp_v = NULL): the plan must then hold one tile per request (split_pages None).  Nothing is read
    back from the device."""
    name = "flashinfer_decode"
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{name}: only f16 / bf16 queries are supported, got {q.dtype}")
    code = _fi_cache(name, q.dtype, key_cache, value_cache, k_scale, v_scale)
    request_indices, kv_tile_indices, o_indptr, kv_chunk_size, block_valid_mask = plan
    meta = dict(paged_kv_indptr=paged_kv_indptr, paged_kv_indices=paged_kv_indices, paged_kv_last_page_len=paged_kv_last_page_len,
                request_indices=request_indices, kv_tile_indices=kv_tile_indices, o_indptr=o_indptr, kv_chunk_size=kv_chunk_size)
    for what, t in meta.items():
        if t.dtype != torch.int32:
            raise ValueError(f"{name} expects {what} to be i32")
    if block_valid_mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{name} expects block_valid_mask to be u8")
    meta["block_valid_mask"] = block_valid_mask
    if q.dim() != 3 or not q.is_cuda or q.stride(2) != 1:
        raise ValueError(f"{name}: q must be a GPU tensor [batch, heads, head_size] with contiguous rows, got {tuple(q.shape)}")
    batch, num_heads, head_size = q.shape
    _, num_kv_heads, page_size, cache_head_size = key_cache.shape
    if cache_head_size != head_size:
        raise ValueError(f"{name} cache shape {tuple(key_cache.shape)} incompatible with query {tuple(q.shape)}")
    if any(t.dim() != 1 or not t.is_cuda for t in meta.values()):
        raise ValueError(f"{name}: the request lists and the plan must be GPU vectors")
    padded = request_indices.numel()
    if (paged_kv_indptr.numel() != batch + 1 or paged_kv_last_page_len.numel() != batch or padded < batch or kv_tile_indices.numel() != padded
            or o_indptr.numel() != batch + 1 or kv_chunk_size.numel() != 1 or block_valid_mask.numel() != padded):
        raise ValueError(f"{name} metadata shapes are invalid")
    if num_kv_heads < 1 or num_heads % num_kv_heads:
        raise ValueError(f"{name}: {num_heads} heads are not a multiple of {num_kv_heads} kv heads")
    if head_size not in _FI_HEAD_SIZES or page_size not in (16, 32) or num_heads // num_kv_heads > 16:
        raise ValueError(f"{name}: head_size must be 64 / 128 / 256, page size 16 / 32 and heads / kv_heads <= 16, got {head_size}, {page_size}, "
                         f"{num_heads // num_kv_heads}")
    if window_left is not None and window_left < 0:
        raise ValueError(f"{name}: window_left must be >= 0 or None")
    if logits_soft_cap is not None and not (math.isfinite(logits_soft_cap) and logits_soft_cap > 0.0):
        raise ValueError(f"{name}: logits_soft_cap must be finite and positive, or None")
    meta = {k: t.contiguous() for k, t in meta.items()}
    out = torch.empty(batch, num_heads, head_size, dtype=q.dtype, device=q.device)
    tmp_v = tmp_s = None
    if partition:  # f32 partials [padded, heads, head_size] and their log-sum-exp [padded, heads]
        v_bytes = padded * num_heads * head_size * 4
        tmp_v = _workspace(q.device, v_bytes + padded * num_heads * 4).data_ptr()
        tmp_s = tmp_v + v_bytes
    fn = _lib.sym("paged_attn", "flashinfer_decode", [_vp] * 14 + [_i] * 8 + [_f, _i, _f, _f, _f, _u, _u, _vp], C.c_int32)
    rc = fn(q.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), meta["paged_kv_indptr"].data_ptr(), meta["paged_kv_indices"].data_ptr(),
            meta["paged_kv_last_page_len"].data_ptr(), meta["request_indices"].data_ptr(), meta["kv_tile_indices"].data_ptr(),
            meta["o_indptr"].data_ptr(), meta["kv_chunk_size"].data_ptr(), meta["block_valid_mask"].data_ptr(), out.data_ptr(), tmp_v, tmp_s, batch,
            padded, num_heads, num_kv_heads, head_size, page_size, q.stride(0), q.stride(1), sm_scale, -1 if window_left is None else window_left,
            0.0 if logits_soft_cap is None else logits_soft_cap, k_scale, v_scale, _CODE[q.dtype], code, _stream())
    if rc != 0:
        raise ValueError(f"{name}: flashinfer_decode returned {rc}")
    return out


def prefill_attention(q: torch.Tensor, key_cache: torch.Tensor, value_cache: torch.Tensor, block_table: torch.Tensor, start_pos: int,
                      softmax_scale: float) -> torch.Tensor:
    """Causal prompt attention on the matrix cores (mrs_prefill_attention_f32_bf16): f32 q [T, heads, hd] at positions
    start_pos .. start_pos+T-1 over the bf16 paged cache of ONE sequence (block_table [max_blocks] int32; keys 0 .. start_pos+T-1
    already scattered with reshape_and_cache) -> f32 [T, heads, hd].  Role of Sdpa::run_attention in the prompt branch of
    PagedAttention::forward (paged_attention.rs:1413-1475).  Raises ValueError for shapes the kernel refuses."""
    if q.dtype != torch.float32 or key_cache.dtype != torch.bfloat16 or q.dim() != 3 or not q.is_contiguous():
        raise ValueError("prefill_attention: contiguous f32 query [T, heads, hd] over a bf16 cache")
    T, num_heads, head_size = q.shape
    nb, kvh, hs_x, block_size, x = key_cache.shape
    if block_table.dim() != 1 or block_table.numel() * block_size < start_pos + T:
        raise ValueError("prefill_attention: block_table does not cover start_pos + T tokens")
    out = torch.empty_like(q)
    fn = _lib.sym("ext", "mrs_prefill_attention_f32_bf16", [_vp] * 5 + [_i] * 10 + [_f, _vp], _i)
    rc = fn(q.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), block_table.data_ptr(), out.data_ptr(), T, start_pos, num_heads, kvh,
            head_size, block_size, q.stride(0), out.stride(0), key_cache.stride(0), key_cache.stride(1), softmax_scale, _stream())
    if rc != 0:
        raise ValueError("prefill_attention: unsupported shape (bf16 cache, block_size 32, head_size 128, heads/kv_heads in 1/2/4/8)")
    return out
