"""Host-side mirror of `GptqLayer` (mistralrs-quant/src/gptq/gptq_cuda.rs, gptq_cpu.rs) over the native GPTQ / AWQ entry points of libmrs_hip_ext.so
(`mrs_gptq_matmul`, `mrs_gptq_reconstruct`, `mrs_awq_repack`); the reference's own symbols (`reconstruct_gptq`, `gemm_half_q_half_alt`) sit in
libmistralrsquant.so.

    layer = GptqLayer.from_parts(qweight, qzeros, scales, g_idx, bias, bits)                 # a GPTQ checkpoint's tensors, on the GPU
    layer = GptqLayer.from_parts(qweight, qzeros, scales, None, bias, bits, is_awq=True)     # an AWQ checkpoint's: repacked once, here
    layer = gptq_linear(in_dim, out_dim, config, tensors, prefix)                            # the loader, from a dict of tensors
    y     = layer.forward(x)                                                                 # x [..., K] any float dtype -> [..., N] in x's dtype, through f16
    w_hat = layer.dequantize_w()                                                             # [N, K] f16

Format (GPTQ layout): qweight i32 [K * bits / 32, N], column n holds its K codes as one little-endian bit stream down the rows (3-bit codes 10 and 21 of every
32 straddle two words); qzeros i32 [G, N * bits / 32], the same stream along N; scales f16 [G, N]; g_idx i32 [K], any map from row to group (act-order);
bits in {2, 3, 4, 8}.  W[k][n] = f16_rne((q - (z + 1)) * s), z + 1 not wrapped.  AWQ: qweight i32 [K, N * bits / 32] and qzeros [G, N * bits / 32] packed along
N with the in-word order {0,4,1,5,2,6,3,7} (4 bits) / {0,2,1,3} (8 bits), no g_idx (group = k // group_size), W = f16_rne((q - z) * s); bits 4 / 8.  After
`awq_repack` an AWQ layer is a GPTQ-layout layer with zero offset 0.  y = f16_rne(sum_k x W + bias) with f32 accumulation: the bias joins before the one
rounding (the reference rounds the matmul first, then adds).  PyTorch owns the buffers, every computation is a HIP kernel; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

GPTQ_BITS = (2, 3, 4, 8)
AWQ_BITS = (4, 8)
ROUTES = {1: "gemv", 2: "mfma_tile"}
_I32 = (torch.int32, torch.uint32)

_MATMUL_ARGS = [C.c_void_p] * 7 + [C.c_int] * 6 + [C.c_void_p]
_RECON_ARGS = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]
_REPACK_ARGS = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]


def check_bits(bits, is_awq: bool = False) -> int:
    if bits not in (AWQ_BITS if is_awq else GPTQ_BITS):
        raise ValueError(f"Invalid {'AWQ' if is_awq else 'GPTQ'} bits {bits}.")
    return int(bits)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("gptq: tensors must live on the GPU (no CPU fallback in this package)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rc(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def last_route() -> int:
    """Route code of the last GPTQ matmul launch (see ROUTES and csrc/gptq.hip)."""
    return int(_lib.sym("quant", "gptq_last_route", [], C.c_int)())


def check_parts(qweight, qzeros, scales, g_idx, bits: int, group_size: int | None = None, check_g_idx: bool = True):
    """The shape rules of the GPTQ layout; returns (K, N, G).  Every error names the offending dimension."""
    bits = check_bits(bits)
    if qweight.dtype not in _I32 or qzeros.dtype not in _I32 or g_idx.dtype not in _I32:
        raise ValueError(f"GPTQ qweight, qzeros and g_idx must be i32, got {qweight.dtype}, {qzeros.dtype} and {g_idx.dtype}")
    if scales.dtype != torch.float16:
        raise ValueError(f"GPTQ scales must be f16, got {scales.dtype}")
    if qweight.dim() != 2 or qzeros.dim() != 2 or scales.dim() != 2 or g_idx.dim() != 1:
        raise ValueError(f"GPTQ expects qweight [K * bits / 32, N], qzeros [G, N * bits / 32], scales [G, N] and g_idx [K], got {list(qweight.shape)}, "
                         f"{list(qzeros.shape)}, {list(scales.shape)} and {list(g_idx.shape)}")
    if (qweight.shape[0] * 32) % bits:
        raise ValueError(f"GPTQ qweight has {qweight.shape[0]} rows, which is not a whole number of {bits}-bit codes")
    k, n, g = qweight.shape[0] * 32 // bits, qweight.shape[1], scales.shape[0]
    if k % 32:
        raise ValueError(f"GPTQ in_features K = {k} must be a multiple of 32")
    if n % 32:
        raise ValueError(f"GPTQ out_features N = {n} must be a multiple of 32")
    if group_size is None:
        if g == 0 or k % g:
            raise ValueError(f"GPTQ in_features K = {k} is not divisible into G = {g} groups")
        group_size = k // g
    if group_size <= 0 or k % group_size:
        raise ValueError(f"GPTQ in_features K = {k} must be a multiple of group_size = {group_size}")
    if g != k // group_size:
        raise ValueError(f"GPTQ scales have G = {g} groups, expected K / group_size = {k // group_size}")
    if tuple(scales.shape) != (g, n):
        raise ValueError(f"GPTQ scales must be [G, N] = [{g}, {n}], got {list(scales.shape)}")
    if tuple(qzeros.shape) != (g, n * bits // 32):
        raise ValueError(f"GPTQ qzeros must be [G, N * bits / 32] = [{g}, {n * bits // 32}], got {list(qzeros.shape)}")
    if g_idx.shape[0] != k:
        raise ValueError(f"GPTQ g_idx must have K = {k} entries, got {g_idx.shape[0]}")
    if check_g_idx and k:
        gi = g_idx.view(torch.int32) if g_idx.dtype == torch.uint32 else g_idx
        lo, hi = int(gi.min()), int(gi.max())
        if lo < 0 or hi >= g:
            raise ValueError(f"GPTQ g_idx value {lo if lo < 0 else hi} is outside [0, G = {g})")
    return k, n, g


def awq_repack(qweight: torch.Tensor, qzeros: torch.Tensor, bits: int, group_size: int):
    """AWQ qweight [K, N * bits / 32] and qzeros [G, N * bits / 32] -> (qweight [K * bits / 32, N], qzeros [G, N * bits / 32], g_idx [K]) in GPTQ layout:
    the interleave undone, the code packing moved from along N to along K, g_idx[k] = k // group_size.  Bit exact; the zero points keep their values, so the
    result is used with zero offset 0."""
    bits = check_bits(bits, is_awq=True)
    if qweight.dtype not in _I32 or qzeros.dtype not in _I32:
        raise ValueError(f"AWQ qweight and qzeros must be i32, got {qweight.dtype} and {qzeros.dtype}")
    if qweight.dim() != 2 or qzeros.dim() != 2:
        raise ValueError(f"AWQ expects qweight [K, N * bits / 32] and qzeros [G, N * bits / 32], got {list(qweight.shape)} and {list(qzeros.shape)}")
    pack = 32 // bits
    k, n, g = qweight.shape[0], qweight.shape[1] * pack, qzeros.shape[0]
    if k % 32:
        raise ValueError(f"AWQ in_features K = {k} must be a multiple of 32")
    if n % 32:
        raise ValueError(f"AWQ out_features N = {n} must be a multiple of 32")
    if group_size <= 0 or k % group_size:
        raise ValueError(f"AWQ in_features K = {k} must be a multiple of group_size = {group_size}")
    if g != k // group_size:
        raise ValueError(f"AWQ qzeros have G = {g} groups, expected K / group_size = {k // group_size}")
    if qzeros.shape[1] != n // pack:
        raise ValueError(f"AWQ qzeros must be [G, N * bits / 32] = [{g}, {n // pack}], got {list(qzeros.shape)}")
    _need_gpu(qweight, qzeros)
    qweight, qzeros = qweight.contiguous(), qzeros.contiguous()
    qw = torch.empty(k // pack, n, dtype=torch.int32, device=qweight.device)
    qz = torch.empty(g, n // pack, dtype=torch.int32, device=qweight.device)
    gi = torch.empty(k, dtype=torch.int32, device=qweight.device)
    _rc(_lib.sym("ext", "mrs_awq_repack", _REPACK_ARGS, C.c_int)(qweight.data_ptr(), qzeros.data_ptr(), qw.data_ptr(), qz.data_ptr(), gi.data_ptr(), k, n, g,
                                                                 int(group_size), bits, _stream()), "mrs_awq_repack")
    return qw, qz, gi


def reconstruct(qweight, qzeros, scales, g_idx, bits: int, zero_offset: int = 1, out: torch.Tensor | None = None, validate: bool = True) -> torch.Tensor:
    """`reconstruct_gptq`: the dense f16 [K, N] weight, W[k][n] = f16_rne((q - (z + zero_offset)) * s)."""
    k, n, g = check_parts(qweight, qzeros, scales, g_idx, bits, check_g_idx=validate)
    _need_gpu(qweight, qzeros, scales, g_idx, out)
    if zero_offset not in (0, 1):
        raise ValueError(f"GPTQ zero_offset must be 0 (AWQ) or 1 (GPTQ), got {zero_offset}")
    qweight, qzeros, scales, g_idx = qweight.contiguous(), qzeros.contiguous(), scales.contiguous(), g_idx.contiguous()
    if out is None:
        out = torch.empty(k, n, dtype=torch.float16, device=qweight.device)
    elif tuple(out.shape) != (k, n) or out.dtype != torch.float16 or not out.is_contiguous():
        raise ValueError(f"gptq: `out` must be a contiguous f16 tensor of shape [{k}, {n}]")
    _rc(_lib.sym("ext", "mrs_gptq_reconstruct", _RECON_ARGS, C.c_int)(qweight.data_ptr(), qzeros.data_ptr(), scales.data_ptr(), g_idx.data_ptr(), out.data_ptr(), k, n,
                                                                      g, int(bits), int(zero_offset), _stream()), "mrs_gptq_reconstruct")
    return out


def matmul(x: torch.Tensor, qweight, qzeros, scales, g_idx, bits: int, bias: torch.Tensor | None = None, zero_offset: int = 1, out: torch.Tensor | None = None,
           validate: bool = True) -> torch.Tensor:
    """x f16 [M, K] -> f16 [M, N] = f16_rne(sum_k x W + bias): route 1 (GEMV) for M <= 8, route 2 (MFMA tile) above.  `validate=False` skips the g_idx range
    check (a device read), for callers that checked the tensors once."""
    k, n, g = check_parts(qweight, qzeros, scales, g_idx, bits, check_g_idx=validate)
    _need_gpu(x, qweight, qzeros, scales, g_idx, bias, out)
    if x.dtype != torch.float16:
        raise ValueError(f"GPTQ matmul expects f16 activations, got {x.dtype}")
    if x.dim() != 2 or x.shape[1] != k:
        raise ValueError(f"GPTQ matmul expects x [M, K = {k}], got {list(x.shape)}")
    if zero_offset not in (0, 1):
        raise ValueError(f"GPTQ zero_offset must be 0 (AWQ) or 1 (GPTQ), got {zero_offset}")
    if bias is not None and (bias.dtype != torch.float16 or tuple(bias.shape) != (n,)):
        raise ValueError(f"Bias mismatch: expected f16 [{n}], got {bias.dtype} {list(bias.shape)}")
    m = x.shape[0]
    x, qweight, qzeros, scales, g_idx = x.contiguous(), qweight.contiguous(), qzeros.contiguous(), scales.contiguous(), g_idx.contiguous()
    bias = None if bias is None else bias.contiguous()
    if out is None:
        out = torch.empty(m, n, dtype=torch.float16, device=x.device)
    elif tuple(out.shape) != (m, n) or out.dtype != torch.float16 or not out.is_contiguous():
        raise ValueError(f"gptq: `out` must be a contiguous f16 tensor of shape [{m}, {n}]")
    _rc(_lib.sym("ext", "mrs_gptq_matmul", _MATMUL_ARGS, C.c_int)(x.data_ptr(), qweight.data_ptr(), qzeros.data_ptr(), scales.data_ptr(), g_idx.data_ptr(), _ptr(bias),
                                                                 out.data_ptr(), m, n, k, g, int(bits), int(zero_offset), _stream()), "mrs_gptq_matmul")
    return out


class GptqLayer:
    """GPTQ-layout tensors plus the zero offset (1: GPTQ, 0: a repacked AWQ layer).  The tensors are checked once, here."""

    def __init__(self, qweight, qzeros, scales, g_idx, bias=None, bits: int = 4, zero_offset: int = 1, is_awq: bool = False, group_size: int | None = None):
        self.bits = check_bits(bits)
        self.in_features, self.out_features, self.groups = check_parts(qweight, qzeros, scales, g_idx, self.bits, group_size)
        if bias is not None and (bias.dtype != torch.float16 or tuple(bias.shape) != (self.out_features,)):
            raise ValueError(f"Bias mismatch: expected f16 [{self.out_features}], got {bias.dtype} {list(bias.shape)}")
        self.qweight, self.qzeros, self.scales, self.g_idx, self.bias = qweight, qzeros, scales, g_idx, bias
        self.zero_offset, self.is_awq = int(zero_offset), bool(is_awq)
        self.group_size = self.in_features // self.groups

    @classmethod
    def from_parts(cls, qweight, qzeros, scales, g_idx, bias=None, bits: int = 4, is_awq: bool = False, group_size: int | None = None) -> "GptqLayer":
        """`QuantMethodConfig::GptqAwq` without Marlin.  AWQ tensors (`is_awq`, g_idx None) are repacked to the GPTQ layout once, here."""
        if not is_awq:
            if g_idx is None:
                raise ValueError("GPTQ needs g_idx")
            return cls(qweight, qzeros, scales, g_idx, bias, bits, 1, False, group_size)
        bits = check_bits(bits, is_awq=True)
        if g_idx is not None:
            raise ValueError("AWQ has no g_idx")
        if group_size is None:
            if qzeros.dim() != 2 or qweight.dim() != 2 or qzeros.shape[0] == 0 or qweight.shape[0] % qzeros.shape[0]:
                raise ValueError(f"AWQ in_features K = {qweight.shape[0] if qweight.dim() else 0} is not divisible into G = {qzeros.shape[0] if qzeros.dim() else 0} groups")
            group_size = qweight.shape[0] // qzeros.shape[0]
        qw, qz, gi = awq_repack(qweight, qzeros, bits, group_size)
        return cls(qw, qz, scales, gi, bias, bits, 0, True, group_size)

    # ---- QuantMethod surface
    def has_bias(self) -> bool:
        return self.bias is not None

    def dtype_and_device(self):
        return self.scales.dtype, self.scales.device  # gptq_cuda.rs:408-410

    def quantized_act_type(self):
        return torch.float16  # gptq_cuda.rs:400-402

    def name(self) -> str:
        return "gptq"

    def isq_serde_supported(self) -> bool:
        return False

    def dequantize_w(self) -> torch.Tensor:
        """[N, K] f16: reconstruct, transposed.  The reference bails here with a TODO; this is a deliberate addition."""
        return reconstruct(self.qweight, self.qzeros, self.scales, self.g_idx, self.bits, self.zero_offset, validate=False).t().contiguous()

    def forward_raw(self, x: torch.Tensor) -> torch.Tensor:
        """gptq_cuda.rs:357-398: f16 only, leading dims flattened for the matmul and restored."""
        if x.dtype != torch.float16:
            raise ValueError(f"GptqLayer.forward_raw expects f16 activations, got {x.dtype}")
        if x.dim() < 1 or x.shape[-1] != self.in_features:
            raise ValueError(f"GptqLayer expects x [..., K = {self.in_features}], got {list(x.shape)}")
        y = matmul(x.reshape(-1, x.shape[-1]), self.qweight, self.qzeros, self.scales, self.g_idx, self.bits, self.bias, self.zero_offset, validate=False)
        return y.reshape(*x.shape[:-1], self.out_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The trait's `forward` (lib.rs): cast to `quantized_act_type`, `forward_raw`, cast back."""
        return self.forward_raw(x.to(self.quantized_act_type())).to(x.dtype)

    def gather_forward(self, x: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
        raise ValueError(f"{self.name()} does not support `gather_forward`. Please raise an issue.")

    def add_delta_w(self, delta: torch.Tensor):
        raise ValueError("GPTQ quantization does not support adding weight delta.")

    def apply_isq(self, dtype=None, imatrix_weight=None):
        raise ValueError("GPTQ quantization does not support ISQ.")


# ------------------------------------------------------------------------------------------------ loader (a pure function over a dict of tensors)
def _get(tensors: dict, name: str, shape, dtype) -> torch.Tensor:
    if name not in tensors:
        raise ValueError(f"cannot find tensor {name}")
    t = tensors[name]
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"shape mismatch for {name}: expected {list(shape)}, got {list(t.shape)}")
    if t.dtype not in dtype:
        raise ValueError(f"dtype mismatch for {name}: expected {dtype[0]}, got {t.dtype}")
    return t


def gptq_linear(in_dim: int, out_dim: int, config: dict, tensors: dict, prefix: str, device=None):
    """`gptq_linear` (gptq_cpu.rs:83-159, gptq_cuda.rs:451-623) without the Marlin branch.  `config`: `bits`, `group_size`, `quant_method` "gptq" / "awq",
    optional `checkpoint_format`.  A plain `{prefix}.weight` yields the unquantized layer (without a bias, as the reference's `linear_b(.., false, ..)`).
    Otherwise `{prefix}.qweight` i32 [in * bits / 32, out] (AWQ: [in, out * bits / 32]), `.qzeros` i32 [in / group_size, out * bits / 32], `.scales` f16
    [in / group_size, out], `.g_idx` i32 [in] (GPTQ only), optional `.bias` f16 [out].  The 3-bit qweight has in * 3 / 32 rows (the reference's integer pack
    factor 32 / 3 = 10 does not describe a 3-bit checkpoint)."""
    if not isinstance(config, dict) or config.get("quant_method") not in ("gptq", "awq") or "bits" not in config or "group_size" not in config:
        raise ValueError("Unexpected quantization config.")
    is_awq = config["quant_method"] == "awq"
    fmt = config.get("checkpoint_format")
    if fmt == "marlin":
        raise ValueError(f"GPTQ / AWQ checkpoint_format '{fmt}' is not supported: Marlin is an NVIDIA weight layout")
    bits, group = check_bits(config["bits"], is_awq), int(config["group_size"])
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    if f"{prefix}.weight" in tensors:
        from .blockwise_fp8 import UnquantLinear
        return UnquantLinear(to(_get(tensors, f"{prefix}.weight", (out_dim, in_dim), (torch.float16, torch.bfloat16, torch.float32))), None)
    if group <= 0 or in_dim % group:
        raise ValueError(f"GPTQ in_features K = {in_dim} must be a multiple of group_size = {group}")
    for name in ("qweight", "qzeros", "scales") + (() if is_awq else ("g_idx",)):
        if f"{prefix}.{name}" not in tensors:
            raise ValueError(f"cannot find tensor {prefix}.{name}")
    g = in_dim // group
    qw_shape = (in_dim, out_dim * bits // 32) if is_awq else (in_dim * bits // 32, out_dim)
    qweight = _get(tensors, f"{prefix}.qweight", qw_shape, _I32)
    qzeros = _get(tensors, f"{prefix}.qzeros", (g, out_dim * bits // 32), _I32)
    g_idx = None if is_awq else _get(tensors, f"{prefix}.g_idx", (in_dim,), _I32)
    scales = _get(tensors, f"{prefix}.scales", (g, out_dim), (torch.float16,))
    bias = _get(tensors, f"{prefix}.bias", (out_dim,), (torch.float16,)) if f"{prefix}.bias" in tensors else None
    return GptqLayer.from_parts(to(qweight), to(qzeros), to(scales), None if g_idx is None else to(g_idx), None if bias is None else to(bias), bits, is_awq, group)
