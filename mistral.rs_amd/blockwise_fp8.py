"""Host-side mirror of `BlockwiseFP8Linear` (mistralrs-quant/src/blockwise_fp8/mod.rs, ops.rs) over the drop-in blockwise-FP8 C ABI of libmistralrsquant.so
(`launch_dequant_fp8_blockwise_kernel_*`, `launch_quant_fp8_blockwise_kernel_*`, `launch_fp8_matmul_*`, `launch_fp8_indexed_moe_gemm_*`).

    layer = BlockwiseFP8Linear(weight, weight_scale_inv, bias)    # weight u8 / float8_e4m3fn [N, K], or [E, N, K] for stacked experts
    layer = BlockwiseFP8Linear.quantize(w, (128, 128))            # dense [N, K] f32 / f16 / bf16 -> E4M3 bytes + one f32 scale per block
    y     = layer.forward(x)                                      # x [..., K] f16 / bf16 -> [..., N]
    y     = layer.gather_forward(x, indices)                      # x [T, K], [T, 1, K] or [T, topk, K], indices [T, topk] -> [T, topk, N]
    w_hat = layer.dequantize_w()                                  # dequant_dtype
    other = layer.apply_isq(GgmlDType.Q4K)                        # dequantize, then re-quantize (GGML types, "HQQ4" / "HQQ8", "MXFP4", or None for dense)

Format (HF `quantization_config: {quant_method: fp8, fmt: e4m3, weight_block_size: [bsy, bsx]}`): OCP E4M3FN weight bytes; `weight_scale_inv` f32
[ceil(N / bsy), ceil(K / bsx)], element (n, k) is f32(byte) * scale[n // bsy, k // bsx].  The loader pieces (`scale_shard_from_weight_shard`,
`blockwise_fp8_module_kind`, `blockwise_fp8_linear_b`, `blockwise_fp8_moe`) are pure functions over a dict of checkpoint tensors.  PyTorch owns the buffers;
every computation is a HIP kernel.  No CPU fallback: apart from the loader's shape logic, tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .distributed import Shard

FP8_E4M3_MAX = 448.0
_TAG = {torch.float16: "f16", torch.bfloat16: "bf16"}
_TAG3 = {torch.float32: "f32", **_TAG}
ROUTES = {1: "gemv", 2: "mfma_tile", 3: "moe_per_slot", 4: "moe_grouped_tile", 5: "general"}
HQQ_ISQ_GROUP_SIZE = 64  # ISQ_HQQ_GROUP_SIZE (lib.rs)
_F8 = getattr(torch, "float8_e4m3fn", None)

_DQ_ARGS = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
_MATMUL_ARGS = [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p]
_MOE_ARGS = [C.c_void_p] * 5 + [C.c_int] * 8 + [C.c_bool, C.c_void_p]


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("blockwise_fp8: tensors must live on the GPU (no CPU fallback in this package)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def last_route() -> int:
    """Route code of the last blockwise-FP8 matmul / MoE launch (see ROUTES and csrc/blockwise_fp8.hip)."""
    return int(_lib.sym("quant", "fp8_blockwise_last_route", [], C.c_int)())


def _block(block_size) -> tuple[int, int]:
    bs = [int(b) for b in block_size]
    if len(bs) != 2:
        raise ValueError(f"Expected weight_block_size to have length 2, got {bs}")
    if 0 in bs or min(bs) < 0:
        raise ValueError(f"Expected nonzero weight_block_size, got {bs}")
    return bs[0], bs[1]


def _as_bytes(weight: torch.Tensor) -> torch.Tensor:
    if weight.dtype == torch.uint8:
        return weight
    if _F8 is not None and weight.dtype == _F8:
        return weight.view(torch.uint8)
    raise ValueError(f"Expected the weight as u8 or float8_e4m3fn bytes, got {weight.dtype}")


def _scale_shape(shape, bs):
    return (*shape[:-2], -(-shape[-2] // bs[0]), -(-shape[-1] // bs[1]))


def dequantize(weight: torch.Tensor, scale: torch.Tensor, block_size, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """`fp8_blockwise_dequantize` (ops.rs): weight [H, W] (or [E, H, W]) E4M3 bytes, scale f32 [ceil(H / bsy), S >= ceil(W / bsx)] -> T(f32(w) * scale)."""
    weight = _as_bytes(weight)
    _need_gpu(weight, scale)
    bs = _block(block_size)
    if dtype not in _TAG3:
        raise ValueError(f"Unsupported dtype for blockwise FP8 dequantize: {dtype}")
    if weight.dim() not in (2, 3):
        raise ValueError(f"Expected weight to be rank 2 (or 3 for stacked experts), got {list(weight.shape)}")
    want = _scale_shape(weight.shape, bs)
    if scale.dim() != weight.dim() or scale.dtype != torch.float32 or tuple(scale.shape[:-1]) != want[:-1] or scale.shape[-1] < want[-1]:
        raise ValueError(f"Scale shape mismatch: expected f32 {list(want)}, got {scale.dtype} {list(scale.shape)}")
    weight, scale = weight.contiguous(), scale.contiguous()
    out = torch.empty(weight.shape, dtype=dtype, device=weight.device)
    h, w = weight.shape[-2:]
    if weight.numel():
        fn = _lib.sym("quant", f"launch_dequant_fp8_blockwise_kernel_{_TAG3[dtype]}", _DQ_ARGS)
        for wi, si, oi in ((weight, scale, out),) if weight.dim() == 2 else zip(weight, scale, out):  # every expert has its own scale rows
            fn(wi.data_ptr(), si.data_ptr(), oi.data_ptr(), h, w, w, scale.shape[-1], bs[0], bs[1], _stream())
    return out


def quantize_tensors(w: torch.Tensor, block_size, scale_row_stride: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """`fp8_blockwise_quantize` (ops.rs:628-): w [H, W] f32 / f16 / bf16 on the GPU -> (E4M3 bytes u8 [H, W], scale f32 [ceil(H / bsy), ceil(W / bsx)]).
    `scale_row_stride` (>= ceil(W / bsx), the ABI's scale_stride) widens the scale rows; the extra columns stay zero."""
    _need_gpu(w)
    bs = _block(block_size)
    if w.dim() != 2:
        raise ValueError("Expected input to be rank 2")
    if w.dtype not in _TAG3:
        raise ValueError(f"unexpected input type for fp8 blockwise quant: {w.dtype}")
    w = w.contiguous()
    h, wd = w.shape
    gy, gx = _scale_shape(w.shape, bs)
    q = torch.zeros(h, wd, dtype=torch.uint8, device=w.device)
    stride = gx if scale_row_stride is None else int(scale_row_stride)
    if stride < gx:
        raise ValueError(f"scale_row_stride {stride} is smaller than the {gx} blocks of a row")
    scale = torch.zeros(gy, stride, dtype=torch.float32, device=w.device)
    if h and wd:
        _lib.sym("quant", f"launch_quant_fp8_blockwise_kernel_{_TAG3[w.dtype]}", _DQ_ARGS)(
            w.data_ptr(), q.data_ptr(), scale.data_ptr(), h, wd, wd, stride, bs[0], bs[1], _stream())
    return q, scale


def matmul(x: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor, block_size) -> torch.Tensor:
    """`fp8_blockwise_matmul` (ops.rs): x [M, K] f16 / bf16 (any element-aligned view), weight [N, K] bytes, scale f32 [ceil(N / bsy), S >= ceil(K / bsx)] -> [M, N]."""
    weight = _as_bytes(weight)
    _need_gpu(x, weight, scale)
    bs = _block(block_size)
    if x.dim() != 2:
        raise ValueError(f"Expected input to be rank 2, got {list(x.shape)}")
    if x.dtype not in _TAG:
        raise ValueError(f"Unsupported dtype for blockwise FP8 matmul: {x.dtype}")
    m, k = x.shape
    if weight.dim() != 2 or weight.shape[1] != k:
        raise ValueError(f"Weight shape mismatch: expected [N, K] = [N, {k}], got {list(weight.shape)}")
    n = weight.shape[0]
    gy, gx = _scale_shape(weight.shape, bs)
    if scale.dim() != 2 or scale.dtype != torch.float32 or scale.shape[0] != gy or scale.shape[1] < gx:
        raise ValueError(f"Scale shape mismatch: expected f32 [{gy}, {gx}], got {scale.dtype} {list(scale.shape)}")
    x, weight, scale = x.contiguous(), weight.contiguous(), scale.contiguous()
    out = torch.empty(m, n, dtype=x.dtype, device=x.device)
    if m and n:
        _lib.sym("quant", f"launch_fp8_matmul_{_TAG[x.dtype]}", _MATMUL_ARGS)(
            x.data_ptr(), weight.data_ptr(), scale.data_ptr(), out.data_ptr(), m, n, k, scale.shape[1], bs[0], bs[1], _stream())
    return out


def indexed_moe_gemm(x: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor, indices: torch.Tensor, block_size, out: torch.Tensor | None = None) -> torch.Tensor:
    """`fp8_indexed_moe_gemm` (ops.rs:945-): x [T, K], [T, 1, K] or [T, topk, K]; weight [E, N, K] bytes; scale f32 [E, ceil(N / bsy), S]; indices [T, topk] read
    as u32 -> [T, topk, N].  Rows whose expert id is >= E keep what `out` held (zeros when `out` is not given, as the reference's alloc_zeros)."""
    weight = _as_bytes(weight)
    _need_gpu(x, weight, scale, indices)
    bs = _block(block_size)
    if indices.dim() != 2:
        raise ValueError(f"Expected indices to be rank 2 [num_tokens, topk], got {list(indices.shape)}")
    t, topk = indices.shape
    if x.dim() == 3 and x.shape[1] == 1:
        x = x.reshape(x.shape[0], x.shape[2])
    if x.dim() == 2:
        k, has_topk = x.shape[1], False
    elif x.dim() == 3:
        k, has_topk = x.shape[2], True
        if x.shape[1] != topk:
            raise ValueError(f"Input shape mismatch: expected [{t}, {topk}, K] or [{t}, 1, K], got {list(x.shape)}")
    else:
        raise ValueError(f"Expected input to be rank 2 or 3, got {list(x.shape)}")
    if x.shape[0] != t:
        raise ValueError(f"Indices shape mismatch: expected [{x.shape[0]}, topk], got {list(indices.shape)}")
    if x.dtype not in _TAG:
        raise ValueError(f"Unsupported dtype for blockwise FP8 indexed MoE GEMM: {x.dtype}")
    if weight.dim() != 3 or weight.shape[2] != k:
        raise ValueError(f"Weight shape mismatch: expected [num_experts, N, K], got {list(weight.shape)}")
    e, n = weight.shape[0], weight.shape[1]
    _, gy, gx = _scale_shape(weight.shape, bs)
    if scale.dim() != 3 or scale.dtype != torch.float32 or scale.shape[0] != e or scale.shape[1] != gy or scale.shape[2] < gx:
        raise ValueError(f"Scale shape mismatch: expected f32 [{e}, {gy}, {gx}], got {scale.dtype} {list(scale.shape)}")
    x, weight, scale = x.contiguous(), weight.contiguous(), scale.contiguous()
    idx = indices.to(torch.int64).to(torch.int32).contiguous()  # u32 ids: the same 32 bits
    if out is None:
        out = torch.zeros(t, topk, n, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (t, topk, n) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError(f"blockwise_fp8: `out` must be a contiguous {x.dtype} tensor of shape [{t}, {topk}, {n}]")
    if t and topk and n:
        _lib.sym("quant", f"launch_fp8_indexed_moe_gemm_{_TAG[x.dtype]}", _MOE_ARGS)(
            x.data_ptr(), weight.data_ptr(), scale.data_ptr(), idx.data_ptr(), out.data_ptr(), t, topk, e, n, k, scale.shape[2], bs[0], bs[1], has_topk, _stream())
    return out


class UnquantLinear:
    """The plain dense layer `apply_isq(None)` and an FP8-excluded module become (`UnquantLinear`, unquantized/mod.rs): x @ W^T (+ bias), the library matmul."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor | None = None):
        self.weight, self.bias = weight, bias

    def has_bias(self) -> bool:
        return self.bias is not None

    def dtype_and_device(self):
        return self.weight.dtype, self.weight.device

    def dequantize_w(self) -> torch.Tensor:
        return self.weight

    def name(self) -> str:
        return "unquant-linear"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.nn.functional.linear(x, self.weight.to(x.dtype), None if self.bias is None else self.bias.to(x.dtype))


class BlockwiseFP8Linear:
    def __init__(self, weight: torch.Tensor, weight_scale_inv: torch.Tensor, bias: torch.Tensor | None = None, dequant_dtype: torch.dtype = torch.bfloat16,
                 weight_block_size=(128, 128), activation_scheme: str | None = None):
        weight = _as_bytes(weight)
        bs = _block(weight_block_size)
        if weight.dim() not in (2, 3):
            raise ValueError(f"Blockwise FP8 weight must be [N, K] or [num_experts, N, K], got {list(weight.shape)}")
        if weight_scale_inv.dtype != torch.float32:
            raise ValueError(f"Blockwise FP8 weight_scale_inv must be an f32 tensor, got {weight_scale_inv.dtype}")
        if tuple(weight_scale_inv.shape) != _scale_shape(weight.shape, bs):
            raise ValueError(f"Scale shape mismatch: expected {list(_scale_shape(weight.shape, bs))}, got {list(weight_scale_inv.shape)}")
        if bias is not None and bias.shape[-1] != weight.shape[-2]:
            raise ValueError(f"Bias shape mismatch: expected [..., {weight.shape[-2]}], got {list(bias.shape)}")
        if dequant_dtype not in _TAG3:
            raise ValueError(f"Unsupported dequant_dtype for blockwise FP8: {dequant_dtype}")
        self.weight, self.weight_scale_inv, self.bias = weight, weight_scale_inv, bias
        self.dequant_dtype, self.weight_block_size, self.activation_scheme = dequant_dtype, bs, activation_scheme

    @classmethod
    def quantize(cls, w: torch.Tensor, block_size=(128, 128), bias: torch.Tensor | None = None, dequant_dtype: torch.dtype | None = None) -> "BlockwiseFP8Linear":
        q, scale = quantize_tensors(w, block_size)
        return cls(q, scale, bias, dequant_dtype or (w.dtype if w.dtype in _TAG else torch.bfloat16), block_size)

    # ---- QuantMethod surface
    def has_bias(self) -> bool:
        return self.bias is not None

    def dtype_and_device(self):
        return (_F8 or "F8E4M3"), self.weight.device  # mod.rs: (DType::F8E4M3, device)

    def quantized_act_type(self):
        return None

    def name(self) -> str:
        return "blockwise-fp8-linear"

    def isq_serde_supported(self) -> bool:
        return False  # no UQFF for this layer, as in the reference (mod.rs:673-680)

    def dequantize_w(self) -> torch.Tensor:
        """mod.rs:180-187."""
        return dequantize(self.weight, self.weight_scale_inv, self.weight_block_size, self.dequant_dtype)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """mod.rs:239-279: leading dims are flattened for the matmul and restored; the bias is added afterwards in x's dtype (broadcast_add)."""
        if self.weight.dim() != 2:
            raise ValueError(f"Blockwise FP8 forward expects a rank-2 weight, got {list(self.weight.shape)}; stacked experts go through gather_forward")
        if x.dim() < 2:
            raise ValueError(f"Expected input to be rank 2, got {list(x.shape)}")
        y = matmul(x.reshape(-1, x.shape[-1]), self.weight, self.weight_scale_inv, self.weight_block_size)
        y = y.reshape(*x.shape[:-1], y.shape[1])
        return y if self.bias is None else y + self.bias.to(y.dtype)

    def gather_forward(self, x: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
        """mod.rs:296-317."""
        if self.weight.dim() != 3:
            raise ValueError(f"Weight shape mismatch: expected [num_experts, N, K], got {list(self.weight.shape)}")
        y = indexed_moe_gemm(x, self.weight, self.weight_scale_inv, indices, self.weight_block_size)
        return y if self.bias is None else y + self.bias.to(y.dtype)

    def apply_isq(self, dtype, imatrix_weight=None):
        """mod.rs:501-670: dequantize, then hand the dense weight to the target's quantizer.  `dtype`: a GgmlDType, "HQQ4" / "HQQ8", "MXFP4", or None."""
        from . import hqq, isq, mxfp4
        from .gguf.matmul import GgufMatMul
        from .gguf.qtensor import GgmlDType
        if self.weight.dim() != 2:
            raise ValueError(f"Blockwise FP8 apply_isq expects a rank-2 weight, got {list(self.weight.shape)}")
        weight = self.dequantize_w()
        if dtype in ("HQQ4", "HQQ8"):
            if imatrix_weight is not None:
                raise ValueError("HQQ does not support imatrix.")
            cfg = hqq.HqqConfig(bits=int(dtype[3:]), group_size=HQQ_ISQ_GROUP_SIZE, axis=0, optimization_steps=hqq.OPTIMIZER_HQQ_DEFAULT_STEPS, round_zeros=False,
                                channel_wise=True)
            res = hqq.HqqLayer.quantize(weight, cfg)
            return res if self.bias is None else res.with_bias(self.bias.to(res.scales.dtype))
        if dtype == "MXFP4":
            if imatrix_weight is not None:
                raise ValueError("MXFP4 does not support imatrix.")
            return mxfp4.MXFP4Layer.quantize(weight, self.bias)
        if dtype is None:
            return UnquantLinear(weight, self.bias)  # the imatrix is ignored altogether
        if isinstance(dtype, GgmlDType):
            target = isq.get_quantization_behaviour(weight.shape, dtype)
            if target is None:
                raise ValueError(f"isq: no GGML type fits a weight of shape {list(weight.shape)} for {dtype.name}")
            if imatrix_weight is not None and isq.imatrix_capable(target):
                q = isq.quantize_imatrix(weight, imatrix_weight, target)
            else:
                q = isq.quantize(weight, target)
            return GgufMatMul(q, None if self.bias is None else self.bias.to(torch.float32))
        raise ValueError(f"Blockwise FP8 apply_isq: unsupported ISQ type {dtype!r}")


# ------------------------------------------------------------------------------------------------ loader pieces (pure functions)
def scale_shard_from_weight_shard(weight_shape, block_size, shard: Shard) -> Shard:
    """mod.rs:864-925: the shard of `weight_scale_inv` that belongs to a shard of the rank-2 weight.  The weight range must start on a block boundary and end
    on one or at the dimension's end."""
    weight_shape, block_size = tuple(weight_shape), tuple(block_size)
    dim = shard.dim
    if shard.offset is None:
        if shard.world_size == 0 or shard.rank >= shard.world_size:
            raise ValueError(f"Invalid FP8 weight shard rank {shard.rank} for world size {shard.world_size}")
        if not 0 <= dim < 2:
            raise ValueError(f"Cannot shard rank-2 FP8 weight along dimension {dim}")
        if weight_shape[dim] % shard.world_size:
            raise ValueError(f"FP8 weight dimension {weight_shape[dim]} is not divisible by world size {shard.world_size}")
        length = weight_shape[dim] // shard.world_size
        offset = shard.rank * length
    else:
        offset, length = shard.offset, shard.length
    if not 0 <= dim < 2:
        raise ValueError(f"Cannot shard rank-2 FP8 weight along dimension {dim}")
    logical, bs = weight_shape[dim], block_size[dim]
    if bs == 0:
        raise ValueError("FP8 weight block size must be nonzero")
    end = offset + length
    if end > logical:
        raise ValueError(f"FP8 weight shard {offset}..{end} exceeds dimension size {logical}")
    if offset % bs or (end != logical and end % bs):
        raise ValueError(f"FP8 weight shard {offset}..{end} is not aligned to block size {bs}")
    lo, hi = offset // bs, -(-end // bs)
    return Shard(dim=dim, offset=lo, length=hi - lo)


def _canonical_language_model_module_path(path: str) -> str:
    for prefix in ("model.language_model.", "language_model.model."):
        if path.startswith(prefix):
            return "model." + path[len(prefix):]
    return path


def blockwise_fp8_module_kind(config: dict, names, prefix: str) -> str:
    """mod.rs:786-835: "quantized", "unquantized" or "missing" for the module `prefix`, given the checkpoint's tensor names and its FP8 quantization config
    (`modules_to_not_convert`; `model.language_model.` / `language_model.model.` prefixes are the same module as `model.`)."""
    if not isinstance(config, dict) or config.get("quant_method", "fp8") != "fp8":
        raise ValueError("Unexpected quantization config.")
    excluded = list(config.get("modules_to_not_convert") or [])
    has_weight, has_scale = f"{prefix}.weight" in names, f"{prefix}.weight_scale_inv" in names
    path = _canonical_language_model_module_path(prefix)
    if any(_canonical_language_model_module_path(m) == path for m in excluded):
        if has_scale:
            raise ValueError(f"FP8-excluded module `{prefix}` unexpectedly has `weight_scale_inv`")
        return "unquantized" if has_weight else "missing"
    if has_weight and not has_scale:
        if excluded:
            raise ValueError(f"FP8 module `{prefix}` has no `weight_scale_inv` and is not listed in `modules_to_not_convert`")
        return "unquantized"
    return "quantized" if has_weight and has_scale else "missing"


def _apply_shard(t: torch.Tensor, shard: Shard | None) -> torch.Tensor:
    if shard is None or (shard.offset is None and shard.world_size == 1):
        return t
    lo, hi = shard.bounds(t.shape[shard.dim])
    return t.narrow(shard.dim, lo, hi - lo).contiguous()


def _get(tensors: dict, name: str, shape, shard: Shard | None = None) -> torch.Tensor:
    if name not in tensors:
        raise ValueError(f"cannot find tensor {name}")
    t = tensors[name]
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"shape mismatch for {name}: expected {list(shape)}, got {list(t.shape)}")
    return _apply_shard(t, shard)


def blockwise_fp8_linear_b(in_dim: int, out_dim: int, config: dict, bias: bool, shard: Shard | None, tensors: dict, prefix: str,
                           dtype: torch.dtype = torch.bfloat16, device=None):
    """mod.rs:703-777: the layer of module `prefix` of a blockwise-FP8 checkpoint, `shard` applied to the weight and the matching shard to its scales.
    An excluded (or scale-less, when nothing is declared excluded) module comes back as an UnquantLinear that keeps its shard."""
    shard = shard or Shard()
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    kind = blockwise_fp8_module_kind(config, tensors.keys(), prefix)
    if kind == "missing":
        raise ValueError(f"blockwise_fp8_linear: cannot find tensor {prefix}.weight")
    get_bias = lambda: to(_get(tensors, f"{prefix}.bias", (out_dim,))) if bias else None
    if kind == "unquantized":
        return UnquantLinear(to(_get(tensors, f"{prefix}.weight", (out_dim, in_dim), shard)), get_bias())
    bs = config.get("weight_block_size")
    if bs is None:
        raise ValueError("Blockwise FP8 requires weight_block_size to be set. Use per-tensor FP8 for models without block sizes.")
    bs = list(bs)
    if len(bs) != 2:
        raise ValueError(f"Expected weight_block_size to have length 2, got {bs}")
    if 0 in bs:
        raise ValueError(f"Expected nonzero weight_block_size, got {bs}")
    fmt = config.get("fmt")
    if fmt is not None and fmt != "e4m3":
        raise ValueError(f"Unsupported blockwise FP8 format {fmt!r}; expected `e4m3`")
    scale_shard = scale_shard_from_weight_shard((out_dim, in_dim), bs, shard)
    weight = _as_bytes(_get(tensors, f"{prefix}.weight", (out_dim, in_dim), shard))
    scale = _get(tensors, f"{prefix}.weight_scale_inv", (-(-out_dim // bs[0]), -(-in_dim // bs[1])), scale_shard).to(torch.float32)
    return BlockwiseFP8Linear(to(weight), to(scale), get_bias(), dtype, bs, config.get("activation_scheme"))


def blockwise_fp8_moe(weight: torch.Tensor, weight_scale_inv: torch.Tensor, weight_block_size, activation_scheme: str | None = None,
                      dequant_dtype: torch.dtype = torch.bfloat16) -> BlockwiseFP8Linear:
    """mod.rs:683-701: stacked experts [E, N, K], no bias."""
    return BlockwiseFP8Linear(weight, weight_scale_inv, None, dequant_dtype, weight_block_size, activation_scheme)
