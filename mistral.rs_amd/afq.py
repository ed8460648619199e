"""Host-side mirror of `AfqLayer` (mistralrs-quant/src/afq/mod.rs, ops.rs) over the native AFQ entry points of libmrs_hip_ext.so (`mrs_afq_matmul`,
`mrs_afq_indexed_moe_gemm`, `mrs_afq_dequantize_rows`, `mrs_afq_quantize`); the reference's own symbols (`afq_qmv_*` ...) sit in libmistralrsquant.so.

    layer = AfqLayer.quantize(w, bias, bits=4, group_size=64)        # [N, K] (or [E, N, K]) f32 / f16 / bf16 on the GPU
    layer = AfqLayer.from_parts(w_q, scales, biases, bias, bits, group_size)
    y     = layer.forward(x)                                          # x [..., K] in the layer's dtype -> [..., N]
    y     = layer.gather_forward(x, indices)                          # x [T, K] or [T, topk, K], indices [T, topk] -> [T, topk, N]
    w_hat = layer.dequantize_w()                                      # the dtype of the scales
    rows  = layer.embedding_forward(ids)
    other = layer.apply_isq(GgmlDType.Q4K)                            # None / the same AFQ type: self; else dequantize, then the target's quantizer

Format: w_q u32 [.., N, K * bits / 32], element j of a row in bits [j * bits, (j + 1) * bits) of the row's little-endian bit stream; scales / biases T
[.., N, K / group]; weight = q * scale + bias.  bits in {2, 3, 4, 6, 8}, group in {32, 64, 128}, T in {f32, f16, bf16}.  PyTorch owns the buffers, every
computation is a HIP kernel.  No CPU fallback: apart from the loader's shape checks and the UQFF byte handling, tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

AFQ_BITS = (2, 3, 4, 6, 8)        # AfqBits (mod.rs:17-25)
AFQ_GROUP_SIZES = (32, 64, 128)   # AfqGroupSize (mod.rs:48-55), default 64
_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ROUTES = {1: "gemv", 2: "mfma_tile", 3: "moe_per_slot", 4: "moe_grouped_tile", 5: "gemv_chunks"}
HQQ_ISQ_GROUP_SIZE = 64
_STACKED_GATHER_TARGETS = ("Q4_0", "Q4_1", "Q5_0", "Q5_1", "Q8_0", "Q8_1", "Q2K", "Q3K", "Q4K", "Q5K", "Q6K", "Q8K")

_MATMUL_ARGS = [C.c_void_p] * 6 + [C.c_int] * 6 + [C.c_void_p]
_MOE_ARGS = [C.c_void_p] * 7 + [C.c_int] * 9 + [C.c_void_p]
_DEQ_ARGS = [C.c_void_p] * 4 + [C.c_int64] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
_QUANT_ARGS = [C.c_void_p] * 4 + [C.c_int64] + [C.c_int] * 4 + [C.c_void_p]


def check_bits(bits) -> int:
    if bits not in AFQ_BITS:
        raise ValueError(f"Invalid AFQ bits {bits}.")
    return int(bits)


def check_group_size(group_size) -> int:
    if group_size not in AFQ_GROUP_SIZES:
        raise ValueError(f"Invalid AFQ group size {group_size}.")
    return int(group_size)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("afq: tensors must live on the GPU (no CPU fallback in this package)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rc(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def last_route() -> int:
    """Route code of the last AFQ matmul / MoE launch (see ROUTES and csrc/afq.hip)."""
    return int(_lib.sym("quant", "afq_last_route", [], C.c_int)())


def _check_parts(w_q, scales, biases, bits, group):
    """The checks of `afq_mm_op` (ops.rs:357-365) on the stored tensors; returns K."""
    if w_q.dtype not in (torch.uint32, torch.int32):
        raise ValueError("AFQ weight matrix must be u32")
    if tuple(scales.shape) != tuple(biases.shape):
        raise ValueError("Scales and biases should have the same shapes")
    if scales.dtype != biases.dtype or scales.dtype not in _CODE:
        raise ValueError(f"Unsupported dtype for AFQ scales and biases: {scales.dtype} and {biases.dtype}")
    if w_q.dim() != scales.dim() or tuple(w_q.shape[:-1]) != tuple(scales.shape[:-1]) or w_q.shape[-1] * 32 // bits != scales.shape[-1] * group or \
            (w_q.shape[-1] * 32) % bits:
        raise ValueError("Last dims of w and scales must be compatible.")
    return scales.shape[-1] * group


def quantize_tensors(w: torch.Tensor, bits: int, group_size: int = 64):
    """`afq_quantize_op` (ops.rs:24-130, the CPU back-end's rule :1534-1622 for every width): w [.., K] -> (w_q u32 [.., K * bits / 32], scales, biases [.., K / group])."""
    bits, group = check_bits(bits), check_group_size(group_size)
    _need_gpu(w)
    if w.dim() < 2:
        raise ValueError("AFQ quantize expects weight matrix of at least rank 2")
    if w.shape[-1] % group:
        raise ValueError(f"Last dim of weight matrix ({list(w.shape)}) must be divisible by group size {group}.")
    if w.dtype not in _CODE:
        raise ValueError(f"Unsupported dtype for AFQ quantize: {w.dtype}")
    w = w.contiguous()
    k = w.shape[-1]
    rows = w.numel() // k
    w_q = torch.empty(*w.shape[:-1], k * bits // 32, dtype=torch.int32, device=w.device)
    scales = torch.empty(*w.shape[:-1], k // group, dtype=w.dtype, device=w.device)
    biases = torch.empty_like(scales)
    _rc(_lib.sym("ext", "mrs_afq_quantize", _QUANT_ARGS, C.c_int)(w.data_ptr(), w_q.data_ptr(), scales.data_ptr(), biases.data_ptr(), rows, k, bits, group,
                                                                  _CODE[w.dtype], _stream()), "mrs_afq_quantize")
    return w_q.view(torch.uint32), scales, biases


def dequantize_rows(w_q, scales, biases, bits: int, group_size: int, ids: torch.Tensor | None = None) -> torch.Tensor:
    """`afq_dequantize_op` / `afq_embedding_op` on rank-2 parts: row r of the result is the dequantized row ids[r] (or r), T(fmaf(q, scale, bias))."""
    bits, group = check_bits(bits), check_group_size(group_size)
    _need_gpu(w_q, scales, biases, ids)
    if w_q.dim() != 2 or scales.dim() != 2 or biases.dim() != 2:
        raise ValueError("AFQ embedding expects 2D weight, scale, and bias tensors")
    r = w_q.shape[0]
    hidden = w_q.shape[-1] * 32 // bits
    if hidden % group or tuple(scales.shape) != (r, hidden // group) or tuple(biases.shape) != (r, hidden // group):
        raise ValueError("Scales and biases do not match the embedding matrix.")
    _check_parts(w_q, scales, biases, bits, group)
    w_q, scales, biases = w_q.contiguous(), scales.contiguous(), biases.contiguous()
    if ids is not None:
        ids = ids.reshape(-1).to(torch.int64)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= r):
            bad = int(ids[(ids < 0) | (ids >= r)][0])
            raise ValueError(f"Embedding id {bad} is out of range for {r} rows.")
        ids = ids.to(torch.int32).contiguous()
    rows = r if ids is None else ids.numel()
    out = torch.empty(rows, hidden, dtype=scales.dtype, device=w_q.device)
    _rc(_lib.sym("ext", "mrs_afq_dequantize_rows", _DEQ_ARGS, C.c_int)(w_q.data_ptr(), scales.data_ptr(), biases.data_ptr(), _ptr(ids), rows, hidden, bits, group,
                                                                       _CODE[scales.dtype], out.data_ptr(), _stream()), "mrs_afq_dequantize_rows")
    return out


def matmul(x: torch.Tensor, w_q, scales, biases, bits: int, group_size: int, bias: torch.Tensor | None = None) -> torch.Tensor:
    """`afq_mm_op` with transpose = true (ops.rs:2942-): x [M, K], w_q [N, K * bits / 32] -> [M, N] (+ bias [N], added in f32 before the one rounding)."""
    bits, group = check_bits(bits), check_group_size(group_size)
    _need_gpu(x, w_q, scales, biases, bias)
    k = _check_parts(w_q, scales, biases, bits, group)
    if x.dim() != 2 or w_q.dim() != 2 or x.shape[1] != k:
        raise ValueError(f"w inner dims ({list(w_q.shape)}) must match x inner dims ({list(x.shape)}). transpose=true")
    if x.dtype != scales.dtype:
        raise ValueError(f"AFQ matmul expects x in the dtype of the scales ({scales.dtype}), got {x.dtype}")
    m, n = x.shape[0], w_q.shape[0]
    x, w_q, scales, biases = x.contiguous(), w_q.contiguous(), scales.contiguous(), biases.contiguous()
    if bias is not None:
        if bias.numel() != n:
            raise ValueError(f"Bias shape mismatch: expected [{n}], got {list(bias.shape)}")
        bias = bias.to(x.dtype).contiguous()
    out = torch.empty(m, n, dtype=x.dtype, device=x.device)
    _rc(_lib.sym("ext", "mrs_afq_matmul", _MATMUL_ARGS, C.c_int)(x.data_ptr(), w_q.data_ptr(), scales.data_ptr(), biases.data_ptr(), _ptr(bias), out.data_ptr(), m, n, k,
                                                                bits, group, _CODE[x.dtype], _stream()), "mrs_afq_matmul")
    return out


def indexed_moe_gemm(x: torch.Tensor, w_q, scales, biases, bits: int, group_size: int, indices: torch.Tensor, bias: torch.Tensor | None = None,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """x [T, K] or [T, topk, K], w_q [E, N, K * bits / 32], scales / biases [E, N, K / group], bias [E, N], indices [T, topk] -> [T, topk, N].  Rows whose
    expert id is >= E keep what `out` held (zeros when `out` is not given)."""
    bits, group = check_bits(bits), check_group_size(group_size)
    _need_gpu(x, w_q, scales, biases, bias, indices)
    k = _check_parts(w_q, scales, biases, bits, group)
    if w_q.dim() != 3:
        raise ValueError(f"Weight shape mismatch: expected [num_experts, N, K * bits / 32], got {list(w_q.shape)}")
    if indices.dim() != 2:
        raise ValueError(f"Expected indices to be rank 2 [num_tokens, topk], got {list(indices.shape)}")
    t, topk = indices.shape
    if x.dim() == 2:
        has_topk = False
    elif x.dim() == 3:
        has_topk = True
        if x.shape[1] != topk:
            raise ValueError(f"Input shape mismatch: expected [{t}, {topk}, K], got {list(x.shape)}")
    else:
        raise ValueError(f"Expected input to be rank 2 or 3, got {list(x.shape)}")
    if x.shape[0] != t or x.shape[-1] != k:
        raise ValueError(f"w inner dims ({list(w_q.shape)}) must match x inner dims ({list(x.shape)}). transpose=true")
    if x.dtype != scales.dtype:
        raise ValueError(f"AFQ matmul expects x in the dtype of the scales ({scales.dtype}), got {x.dtype}")
    e, n = w_q.shape[0], w_q.shape[1]
    x, w_q, scales, biases = x.contiguous(), w_q.contiguous(), scales.contiguous(), biases.contiguous()
    idx = indices.to(torch.int64).to(torch.int32).contiguous()  # u32 ids: the same 32 bits
    if bias is not None:
        if tuple(bias.shape) != (e, n):
            raise ValueError(f"Bias shape mismatch: expected [{e}, {n}], got {list(bias.shape)}")
        bias = bias.to(x.dtype).contiguous()
    if out is None:
        out = torch.zeros(t, topk, n, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (t, topk, n) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError(f"afq: `out` must be a contiguous {x.dtype} tensor of shape [{t}, {topk}, {n}]")
    _rc(_lib.sym("ext", "mrs_afq_indexed_moe_gemm", _MOE_ARGS, C.c_int)(x.data_ptr(), w_q.data_ptr(), scales.data_ptr(), biases.data_ptr(), _ptr(bias), idx.data_ptr(),
                                                                        out.data_ptr(), t, topk, e, n, k, bits, group, _CODE[x.dtype], int(has_topk), _stream()),
        "mrs_afq_indexed_moe_gemm")
    return out


class AfqLayer:
    def __init__(self, w_q: torch.Tensor, scales: torch.Tensor, biases: torch.Tensor, bias: torch.Tensor | None = None, bits: int = 4, group_size: int = 64):
        self.bits, self.group_size = check_bits(bits), check_group_size(group_size)
        if w_q.dtype == torch.int32:
            w_q = w_q.view(torch.uint32)
        if w_q.dim() not in (2, 3):
            raise ValueError(f"AFQ w_q must be [N, K * bits / 32] or [num_experts, N, K * bits / 32], got {list(w_q.shape)}")
        _check_parts(w_q, scales, biases, self.bits, self.group_size)
        if bias is not None and bias.shape[-1] != w_q.shape[-2]:
            raise ValueError(f"Bias shape mismatch: expected [..., {w_q.shape[-2]}], got {list(bias.shape)}")
        self.w_q, self.scales, self.biases, self.bias = w_q, scales, biases, bias

    @classmethod
    def from_parts(cls, w_q, scales, biases, bias=None, bits: int = 4, group_size: int = 64) -> "AfqLayer":
        return cls(w_q, scales, biases, bias, bits, group_size)

    @classmethod
    def quantize(cls, w: torch.Tensor, bias: torch.Tensor | None = None, bits: int = 4, group_size: int = 64) -> "AfqLayer":
        """`QuantMethodConfig::Afq` (mod.rs:158-175)."""
        w_q, scales, biases = quantize_tensors(w, bits, group_size)
        return cls(w_q, scales, biases, bias, bits, group_size)

    # ---- QuantMethod surface
    def has_bias(self) -> bool:
        return self.bias is not None

    def dtype_and_device(self):
        return self.scales.dtype, self.scales.device  # mod.rs:299-301

    def quantized_act_type(self):
        return None

    def name(self) -> str:
        return "afq-layer"

    def isq_serde_supported(self) -> bool:
        return True

    def uqff_type(self) -> str:
        return f"AFQ{self.bits}"

    @property
    def in_features(self) -> int:
        return self.scales.shape[-1] * self.group_size

    def dequantize_w(self) -> torch.Tensor:
        k = self.in_features
        flat = dequantize_rows(self.w_q.reshape(-1, self.w_q.shape[-1]), self.scales.reshape(-1, self.scales.shape[-1]),
                               self.biases.reshape(-1, self.biases.shape[-1]), self.bits, self.group_size)
        return flat.reshape(*self.w_q.shape[:-1], k)

    def embedding_forward(self, ids: torch.Tensor) -> torch.Tensor:
        """`afq_embedding_op` (ops.rs:222-321)."""
        rows = dequantize_rows(self.w_q, self.scales, self.biases, self.bits, self.group_size, ids.to(self.w_q.device))
        return rows.reshape(*ids.shape, self.in_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """`forward_raw` (mod.rs:217-234): leading dims are flattened for the matmul and restored; the bias is added in f32 before the one rounding."""
        if self.w_q.dim() != 2:
            raise ValueError(f"AFQ forward expects a rank-2 weight, got {list(self.w_q.shape)}; stacked experts go through gather_forward")
        if x.dim() < 2:
            raise ValueError(f"Expected input to be rank 2, got {list(x.shape)}")
        y = matmul(x.reshape(-1, x.shape[-1]), self.w_q, self.scales, self.biases, self.bits, self.group_size, self.bias)
        return y.reshape(*x.shape[:-1], y.shape[1])

    def gather_forward(self, x: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
        """`gather_forward_raw` (mod.rs:236-261): a rank-2 bias [E, N] is selected by `indices`; a rank-1 bias [N] is shared by the experts."""
        if self.w_q.dim() != 3:
            raise ValueError(f"Weight shape mismatch: expected [num_experts, N, K * bits / 32], got {list(self.w_q.shape)}")
        bias = self.bias
        if bias is not None and bias.dim() == 1:
            bias = bias.unsqueeze(0).expand(self.w_q.shape[0], -1)
        return indexed_moe_gemm(x, self.w_q, self.scales, self.biases, self.bits, self.group_size, indices, bias)

    def add_delta_w(self, delta: torch.Tensor) -> "AfqLayer":
        """mod.rs:289-297: dequantize, add, quantize again with the same bits and group size."""
        return AfqLayer.quantize(self.dequantize_w() + delta.to(self.scales.dtype), self.bias, self.bits, self.group_size)

    def apply_isq(self, dtype, imatrix_weight=None):
        """mod.rs:303-370.  `dtype`: None, "AFQ2" .. "AFQ8", a GgmlDType, "HQQ4" / "HQQ8" or "MXFP4".  None, or the layer's own type without an imatrix,
        returns self; any other target dequantizes and hands the dense weight to that target's quantizer."""
        if dtype is None or (dtype == self.uqff_type() and imatrix_weight is None):
            return self
        from .gguf.qtensor import GgmlDType
        if self.w_q.dim() == 3 and not (isinstance(dtype, GgmlDType) and dtype.name.upper().replace("_K", "K") in _STACKED_GATHER_TARGETS) \
                and not (isinstance(dtype, str) and dtype.startswith("AFQ")):
            label = dtype.name if isinstance(dtype, GgmlDType) else dtype
            raise ValueError(f"Cannot requantize stacked AFQ expert weights to {label}: that target does not support stacked expert gather. "
                             "Use a Q*K/Q*_0/Q*_1 target, AFQ, or omit ISQ.")
        if dtype == "F8Q8":
            raise ValueError("AFQ apply_isq: F8Q8 is not a requantization target of this package")
        weight = self.dequantize_w()
        if isinstance(dtype, str) and dtype.startswith("AFQ") and dtype[3:].isdigit():
            if imatrix_weight is not None and dtype != self.uqff_type():
                raise ValueError("AFQ does not support imatrix.")
            return AfqLayer.quantize(weight, self.bias, int(dtype[3:]), self.group_size)
        if self.w_q.dim() != 2:
            raise ValueError(f"AFQ apply_isq to {dtype!r} expects a rank-2 weight, got {list(self.w_q.shape)}")
        from . import hqq, isq, mxfp4
        from .gguf.matmul import GgufMatMul
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
        if isinstance(dtype, GgmlDType):
            target = isq.get_quantization_behaviour(weight.shape, dtype)
            if target is None:
                raise ValueError(f"isq: no GGML type fits a weight of shape {list(weight.shape)} for {dtype.name}")
            if imatrix_weight is not None and isq.imatrix_capable(target):
                q = isq.quantize_imatrix(weight, imatrix_weight, target)
            else:
                q = isq.quantize(weight, target)
            return GgufMatMul(q, None if self.bias is None else self.bias.to(torch.float32))
        raise ValueError(f"AFQ apply_isq: unsupported ISQ type {dtype!r}")

    # ---- UQFF (mod.rs:393-432,536-562)
    def serialize_uqff(self, prefix: str) -> dict:
        from . import uqff
        cpu = lambda t: None if t is None else t.detach().cpu().contiguous()
        return uqff.serialize_afq_layer(prefix, cpu(self.w_q), cpu(self.scales), cpu(self.biases), self.bits, self.group_size, cpu(self.bias))

    @classmethod
    def from_uqff(cls, reader, prefix: str, device, shard=None) -> "AfqLayer":
        d = reader.load_afq_layer(prefix, shard)
        to = lambda t: None if t is None else t.to(device)
        return cls(to(d.w_q), to(d.scales), to(d.biases), to(d.bias), d.bits, d.group_size)


# ------------------------------------------------------------------------------------------------ loader pieces (pure functions over a dict of tensors)
def _get(tensors: dict, name: str, shape, dtype=None) -> torch.Tensor:
    if name not in tensors:
        raise ValueError(f"cannot find tensor {name}")
    t = tensors[name]
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"shape mismatch for {name}: expected {list(shape)}, got {list(t.shape)}")
    if dtype is not None and t.dtype not in dtype:
        raise ValueError(f"dtype mismatch for {name}: expected {dtype[0]}, got {t.dtype}")
    return t


def _config(config) -> tuple[int, int]:
    if not isinstance(config, dict) or config.get("quant_method", "afq") != "afq" or "bits" not in config or "group_size" not in config:
        raise ValueError("Unexpected quantization config.")
    return check_bits(config["bits"]), check_group_size(config["group_size"])


def afq_linear_b(in_dim: int, out_dim: int, config: dict, bias: bool, tensors: dict, prefix: str, device=None) -> AfqLayer:
    """mod.rs:434-471: `{prefix}.weight` u32 [out, in * bits / 32], `.scales` / `.biases` [out, in / group], optional `.bias` [out]."""
    bits, group = _config(config)
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    w_q = _get(tensors, f"{prefix}.weight", (out_dim, in_dim * bits // 32), (torch.uint32, torch.int32))
    scales = _get(tensors, f"{prefix}.scales", (out_dim, in_dim // group))
    biases = _get(tensors, f"{prefix}.biases", (out_dim, in_dim // group))
    b = _get(tensors, f"{prefix}.bias", (out_dim,)) if bias else None
    return AfqLayer(to(w_q), to(scales), to(biases), None if b is None else to(b), bits, group)


def afq_packed_linear_b(num_local_experts: int, in_dim: int, out_dim: int, config: dict, bias: bool, tensors: dict, prefix: str, device=None) -> AfqLayer:
    """mod.rs:473-517: the stacked-expert form, every tensor with a leading [num_local_experts]."""
    bits, group = _config(config)
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    e = num_local_experts
    w_q = _get(tensors, f"{prefix}.weight", (e, out_dim, in_dim * bits // 32), (torch.uint32, torch.int32))
    scales = _get(tensors, f"{prefix}.scales", (e, out_dim, in_dim // group))
    biases = _get(tensors, f"{prefix}.biases", (e, out_dim, in_dim // group))
    b = _get(tensors, f"{prefix}.bias", (e, out_dim)) if bias else None
    return AfqLayer(to(w_q), to(scales), to(biases), None if b is None else to(b), bits, group)
