"""Host-side mirror of `BnbLinear` (mistralrs-quant/src/bitsandbytes/mod.rs, op.rs) over the native bitsandbytes entry points of libmrs_hip_ext.so
(`mrs_bnb_dequantize`, `mrs_bnb_matmul`); the reference's nine `dequantize_blockwise_<T>_<type>` symbols sit in libmistralrsquant.so.

    layer = bnb_linear_b(in_dim, out_dim, bias, tensors, prefix, device="cuda")   # the loader, from a dict of checkpoint tensors
    layer = BnbLinear.from_parts(weight, absmax, quant_type, blocksize, (N, K), dtype, bias, nested_absmax, nested_quant_map, nested_blocksize, nested_offset)
    y     = layer.forward(x)                                                      # x [..., K] any float dtype -> [..., N] in x's dtype, through the layer's
    w_hat = layer.dequantize_w()                                                  # [N, K] in the layer's dtype

Format: `weight` u8 is the flat row-major [N, K] tensor, two elements per byte, element 2 i in the high nibble; block b covers flat elements
[b * blocksize, (b + 1) * blocksize).  absmax of block b is f32 absmax[b], or with double quantization (absmax u8)
A_b = f32(f32(nested_quant_map[absmax[b]] * nested_absmax[b // nested_blocksize]) + nested_offset).  W_hat = RNE_T(f32(table[q] * A_b)) with the built-in NF4 /
FP4 table; y = RNE_T(sum_k x W_hat + bias) with f32 accumulation.  The f32 absmax tensor of a double-quantized layer is never materialised: the kernels compute
A_b.  PyTorch owns the buffers, every computation is a HIP kernel; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json

import torch

from . import _lib

SUPPORTED_BLOCKSIZE = [2048, 4096, 1024, 512, 256, 128, 64]  # the reference's order (its error text prints it)
QTYPES = {"int8": 0, "fp4": 1, "nf4": 2}
ROUTES = {1: "gemv", 2: "mfma_tile", 3: "general"}
_TAG = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}

# the published code books as f32, the same literals as csrc/bnb_core.cuh
NF4_TABLE = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
             0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
_FP4_MAG = (0.0, 5.208333333e-03, 0.66666667, 1.0, 0.33333333, 0.5, 0.16666667, 0.25)
FP4_TABLE = _FP4_MAG + tuple(-v for v in _FP4_MAG)  # entry 8 is -0.0

_DEQ_ARGS = [C.c_void_p] * 6 + [C.c_longlong, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p]
_MM_ARGS = [C.c_void_p] * 8 + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_int, C.c_void_p]


def table(quant_type: str) -> torch.Tensor:
    """The built-in 16-entry f32 table of "nf4" or "fp4"."""
    return torch.tensor(NF4_TABLE if quant_type == "nf4" else FP4_TABLE, dtype=torch.float32)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("bnb: tensors must live on the GPU (no CPU fallback in this package)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rc(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def last_route() -> int:
    """Route code of the last bitsandbytes matmul launch (see ROUTES and csrc/bnb.hip)."""
    return int(_lib.sym("quant", "bnb_last_route", [], C.c_int)())


def check_blocksize(blocksize) -> int:
    if blocksize not in SUPPORTED_BLOCKSIZE:
        raise ValueError(f"Blocksize of {blocksize} is not supported, {SUPPORTED_BLOCKSIZE} are.")
    return int(blocksize)


def _check_absmax(numel: int, blocksize: int, absmax, nested_absmax, nested_quant_map, nested_blocksize):
    """The count and dtype rules of the absmax tensors; returns the number of blocks."""
    blocks = -(-numel // blocksize)
    nested = nested_absmax is not None
    if absmax.dtype != (torch.uint8 if nested else torch.float32):
        raise ValueError(f"bnb absmax must be {'u8 (double quantization)' if nested else 'f32'}, got {absmax.dtype}")
    if absmax.numel() != blocks:
        raise ValueError(f"bnb absmax has {absmax.numel()} entries, expected {blocks} blocks of {blocksize}")
    if nested:
        if nested_blocksize is None or int(nested_blocksize) <= 0:
            raise ValueError("`nested_blocksize` must be present.")
        if nested_quant_map is None or nested_quant_map.dtype != torch.float32 or nested_quant_map.numel() != 256:
            raise ValueError("bnb nested_quant_map must be 256 f32 values")
        want = -(-blocks // int(nested_blocksize))
        if nested_absmax.dtype != torch.float32 or nested_absmax.numel() != want:
            raise ValueError(f"bnb nested_absmax has {nested_absmax.numel()} {nested_absmax.dtype} entries, expected {want} f32 blocks of {nested_blocksize}")
    return blocks


def dequantize(weight: torch.Tensor, absmax: torch.Tensor, quant_type: str, blocksize: int, n: int, dtype: torch.dtype = torch.bfloat16,
               code: torch.Tensor | None = None, nested_absmax: torch.Tensor | None = None, nested_quant_map: torch.Tensor | None = None,
               nested_blocksize: int | None = None, nested_offset: float = 0.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """The first `n` elements of a blockwise-quantized u8 tensor as `dtype`, flat.  "nf4" / "fp4": two elements per byte and the built-in table; "int8": one code
    per byte and the caller's 256-entry f32 `code`.  With `nested_absmax` the absmax is u8 and A_b is computed inside the same launch."""
    if quant_type not in QTYPES:
        raise ValueError(f"bnb quant_type must be one of {sorted(QTYPES)}, got {quant_type!r}")
    blocksize = check_blocksize(blocksize)
    if dtype not in _TAG:
        raise ValueError(f"Unsupported bnb dtype {dtype}")
    if weight.dtype != torch.uint8:
        raise ValueError(f"bnb weight must be u8, got {weight.dtype}")
    need = n if quant_type == "int8" else (n + 1) // 2
    if weight.numel() < need:
        raise ValueError(f"bnb weight has {weight.numel()} bytes, {n} elements need {need}")
    if quant_type == "int8" and (code is None or code.dtype != torch.float32 or code.numel() != 256 or nested_absmax is not None):
        raise ValueError("bnb int8 needs a 256-entry f32 code and a plain f32 absmax")
    _check_absmax(n, blocksize, absmax, nested_absmax, nested_quant_map, nested_blocksize)
    _need_gpu(weight, absmax, code, nested_absmax, nested_quant_map, out)
    weight, absmax = weight.contiguous(), absmax.contiguous()
    code = None if code is None else code.contiguous()
    nested_absmax = None if nested_absmax is None else nested_absmax.contiguous()
    nested_quant_map = None if nested_quant_map is None else nested_quant_map.contiguous()
    if out is None:
        out = torch.empty(n, dtype=dtype, device=weight.device)
    elif out.dtype != dtype or out.numel() < n or not out.is_contiguous():
        raise ValueError(f"bnb: `out` must be a contiguous {dtype} tensor of at least {n} elements")
    _rc(_lib.sym("ext", "mrs_bnb_dequantize", _DEQ_ARGS, C.c_int)(weight.data_ptr(), absmax.data_ptr(), _ptr(code), _ptr(nested_absmax), _ptr(nested_quant_map),
                                                                  out.data_ptr(), n, blocksize, int(nested_blocksize or 0), float(nested_offset), QTYPES[quant_type],
                                                                  _TAG[dtype], _stream()), "mrs_bnb_dequantize")
    return out


def matmul(x: torch.Tensor, weight: torch.Tensor, absmax: torch.Tensor, quant_type: str, blocksize: int, n: int, bias: torch.Tensor | None = None,
           nested_absmax: torch.Tensor | None = None, nested_quant_map: torch.Tensor | None = None, nested_blocksize: int | None = None,
           nested_offset: float = 0.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """x T [M, K] -> T [M, N] = RNE_T(sum_k x W_hat + bias), T = x's dtype (f32 / f16 / bf16): route 1 (GEMV) for M <= 8, route 2 (MFMA tile) above for 16-bit
    T, both when K % blocksize == 0; route 3 otherwise."""
    if quant_type not in ("nf4", "fp4"):
        raise ValueError(f"bnb matmul quant_type must be 'nf4' or 'fp4', got {quant_type!r}")
    blocksize = check_blocksize(blocksize)
    if x.dtype not in _TAG:
        raise ValueError(f"Unsupported bnb dtype {x.dtype}")
    if x.dim() != 2:
        raise ValueError(f"bnb matmul expects x [M, K], got {list(x.shape)}")
    m, k = x.shape
    if weight.dtype != torch.uint8 or weight.numel() != (n * k + 1) // 2:
        raise ValueError(f"bnb weight must be {(n * k + 1) // 2} u8 bytes for [{n}, {k}], got {weight.numel()} {weight.dtype}")
    if bias is not None and (bias.dtype != x.dtype or tuple(bias.shape) != (n,)):
        raise ValueError(f"Bias mismatch: expected {x.dtype} [{n}], got {bias.dtype} {list(bias.shape)}")
    _check_absmax(n * k, blocksize, absmax, nested_absmax, nested_quant_map, nested_blocksize)
    _need_gpu(x, weight, absmax, bias, nested_absmax, nested_quant_map, out)
    x, weight, absmax = x.contiguous(), weight.contiguous(), absmax.contiguous()
    bias = None if bias is None else bias.contiguous()
    nested_absmax = None if nested_absmax is None else nested_absmax.contiguous()
    nested_quant_map = None if nested_quant_map is None else nested_quant_map.contiguous()
    if out is None:
        out = torch.empty(m, n, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (m, n) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError(f"bnb: `out` must be a contiguous {x.dtype} tensor of shape [{m}, {n}]")
    floats = int(_lib.sym("quant", "bnb_matmul_workspace_floats", [C.c_int] * 3, C.c_longlong)(m, n, k))
    ws = torch.empty(floats, dtype=torch.float32, device=x.device) if floats else None  # the f32 partials of a K-split GEMV
    _rc(_lib.sym("ext", "mrs_bnb_matmul", _MM_ARGS, C.c_int)(x.data_ptr(), weight.data_ptr(), absmax.data_ptr(), _ptr(nested_absmax), _ptr(nested_quant_map), _ptr(bias),
                                                             out.data_ptr(), _ptr(ws), m, n, k, blocksize, int(nested_blocksize or 0), float(nested_offset),
                                                             QTYPES[quant_type], _TAG[x.dtype], _stream()), "mrs_bnb_matmul")
    return out


class BnbLinear:
    """A 4-bit bitsandbytes layer: packed weight, absmax (plain f32 or double-quantized u8 + nested tensors), optional bias.  Checked once, here."""

    def __init__(self, weight, absmax, quant_type: str, blocksize: int, shape, dtype: torch.dtype, bias=None, nested_absmax=None, nested_quant_map=None,
                 nested_blocksize: int | None = None, nested_offset: float | None = None):
        if quant_type not in ("nf4", "fp4"):
            raise ValueError("Only fp8/nf4 quantization is supported for now.")
        self.blocksize = check_blocksize(blocksize)
        if len(shape) != 2:
            raise ValueError(f"bnb shape must be [N, K], got {list(shape)}")
        self.out_features, self.in_features = int(shape[0]), int(shape[1])
        if dtype not in _TAG:
            raise ValueError(f"Unsupported bnb dtype {dtype}")
        numel = self.out_features * self.in_features
        if weight.dtype != torch.uint8 or weight.numel() != (numel + 1) // 2:
            raise ValueError(f"bnb weight must be {(numel + 1) // 2} u8 bytes for shape {list(shape)}, got {weight.numel()} {weight.dtype}")
        if (nested_absmax is None) != (nested_quant_map is None):
            raise ValueError("bnb nested_absmax and nested_quant_map come together")
        _check_absmax(numel, self.blocksize, absmax, nested_absmax, nested_quant_map, nested_blocksize)
        if nested_absmax is not None and nested_offset is None:
            raise ValueError("`offset` must be present.")
        if bias is not None and tuple(bias.shape) != (self.out_features,):
            raise ValueError(f"Bias mismatch: expected [{self.out_features}], got {list(bias.shape)}")
        self.weight, self.absmax, self.bias = weight.reshape(-1), absmax.reshape(-1), None if bias is None else bias.to(dtype)
        self.nested_absmax = None if nested_absmax is None else nested_absmax.reshape(-1)
        self.nested_quant_map = None if nested_quant_map is None else nested_quant_map.reshape(-1)
        self.nested_blocksize = None if nested_absmax is None else int(nested_blocksize)
        self.nested_offset = 0.0 if nested_absmax is None else float(nested_offset)
        self.quant_type, self.dtype = quant_type, dtype

    @classmethod
    def from_parts(cls, weight, absmax, quant_type, blocksize, shape, dtype, bias=None, nested_absmax=None, nested_quant_map=None, nested_blocksize=None,
                   nested_offset=None) -> "BnbLinear":
        """`QuantMethodConfig::Bnb`."""
        return cls(weight, absmax, quant_type, blocksize, shape, dtype, bias, nested_absmax, nested_quant_map, nested_blocksize, nested_offset)

    def _nested(self):
        return dict(nested_absmax=self.nested_absmax, nested_quant_map=self.nested_quant_map, nested_blocksize=self.nested_blocksize, nested_offset=self.nested_offset)

    # ---- QuantMethod surface
    def has_bias(self) -> bool:
        return self.bias is not None

    def dtype_and_device(self):
        return self.dtype, self.weight.device

    def quantized_act_type(self):
        return None

    def name(self) -> str:
        return "bnb-linear"

    def isq_serde_supported(self) -> bool:
        return False

    def dequantize_w(self) -> torch.Tensor:
        """[N, K] in the layer's dtype; one launch, double quantization included."""
        n = self.out_features * self.in_features
        return dequantize(self.weight, self.absmax, self.quant_type, self.blocksize, n, self.dtype, **self._nested()).view(self.out_features, self.in_features)

    def forward_raw(self, x: torch.Tensor) -> torch.Tensor:
        """x in the layer's dtype, leading dims flattened for the matmul and restored; the bias joins before the one rounding."""
        if x.dtype != self.dtype:
            raise ValueError(f"BnbLinear.forward_raw expects {self.dtype} activations, got {x.dtype}")
        if x.dim() < 1 or x.shape[-1] != self.in_features:
            raise ValueError(f"BnbLinear expects x [..., K = {self.in_features}], got {list(x.shape)}")
        y = matmul(x.reshape(-1, x.shape[-1]), self.weight, self.absmax, self.quant_type, self.blocksize, self.out_features, self.bias, **self._nested())
        return y.reshape(*x.shape[:-1], self.out_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Cast to the layer's dtype, `forward_raw`, cast back (the reference casts the dense weight to x's dtype instead: DESIGN 4.19)."""
        return self.forward_raw(x.to(self.dtype)).to(x.dtype)

    def gather_forward(self, x: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
        raise ValueError(f"{self.name()} does not support `gather_forward`. Please raise an issue.")

    def add_delta_w(self, delta: torch.Tensor):
        raise ValueError("HQQ quantization does not support adding weight delta.")  # the reference's text (bitsandbytes/mod.rs)

    def apply_isq(self, dtype=None, imatrix_weight=None):
        """Dequantize, then the target handling of `BlockwiseFP8Linear.apply_isq`; None gives the dense layer."""
        from .blockwise_fp8 import isq_from_dense
        return isq_from_dense(self.dequantize_w(), self.bias, dtype, imatrix_weight, "bnb")


# ------------------------------------------------------------------------------------------------ loader (a pure function over a dict of tensors)
def bnb_linear_b(in_dim: int, out_dim: int, bias: bool, tensors: dict, prefix: str, device=None) -> BnbLinear:
    """`BnbLinear::linear_b`: `{prefix}.weight` u8, `.weight.quant_state.bitsandbytes__nf4` / `__fp4` (the JSON state as u8 bytes), `.weight.absmax` (f32, or u8
    with `.weight.nested_absmax` and `.weight.nested_quant_map`), `.weight.quant_map`, optional `.bias`.  Every check runs before a tensor is moved to `device`.
    Unlike the reference, which ignores `quant_map` for the 4-bit types, a `quant_map` that is not the built-in table bit for bit raises."""
    wp = f"{prefix}.weight"
    kinds = [t for t in ("nf4", "fp4") if f"{wp}.quant_state.bitsandbytes__{t}" in tensors]
    if not kinds:
        raise ValueError("`BnbLinear` expects either `...__nf4` or `...__fp4` tensors, this means the layer is not 4bit.")
    quant_type = kinds[0]

    def get(name, dtype=None):
        if name not in tensors:
            raise ValueError(f"cannot find tensor {name}")
        if dtype is not None and tensors[name].dtype != dtype:
            raise ValueError(f"dtype mismatch for {name}: expected {dtype}, got {tensors[name].dtype}")
        return tensors[name]

    weight = get(wp, torch.uint8)
    state = json.loads(bytes(get(f"{wp}.quant_state.bitsandbytes__{quant_type}", torch.uint8).cpu().reshape(-1).tolist()).decode("utf-8"))
    blocksize = check_blocksize(state.get("blocksize"))
    if state.get("dtype") not in _DTYPES:
        raise ValueError(f"unknown bnb dtype {state.get('dtype')!r}")
    shape = list(state.get("shape") or [])
    if shape != [out_dim, in_dim]:
        raise ValueError(f"shape mismatch for {wp}: quant_state says {shape}, expected {[out_dim, in_dim]}")
    if weight.numel() != (out_dim * in_dim + 1) // 2:
        raise ValueError(f"bnb weight {wp} has {weight.numel()} bytes, expected {(out_dim * in_dim + 1) // 2} for shape {shape}")
    nested = f"{wp}.nested_absmax" in tensors
    nested_absmax = nested_quant_map = nested_blocksize = nested_offset = None
    if nested:
        nested_blocksize = state.get("nested_blocksize")
        if nested_blocksize is None:
            raise ValueError("`nested_blocksize` must be present.")
        if state.get("nested_dtype") is None:
            raise ValueError("`nested_dtype` must be present.")
        if state.get("nested_offset") is None:
            raise ValueError("`offset` must be present.")
        nested_offset = float(state["nested_offset"])
        nested_absmax, nested_quant_map = get(f"{wp}.nested_absmax", torch.float32), get(f"{wp}.nested_quant_map", torch.float32)
    absmax = get(f"{wp}.absmax", torch.uint8 if nested else torch.float32)
    _check_absmax(out_dim * in_dim, blocksize, absmax, nested_absmax, nested_quant_map, nested_blocksize)
    quant_map = get(f"{wp}.quant_map", torch.float32)
    if quant_map.numel() != 16 or not torch.equal(quant_map.cpu().reshape(-1).view(torch.int32), table(quant_type).view(torch.int32)):
        raise ValueError(f"bnb quant_map of {wp} differs from the built-in {quant_type} table; the kernels decode with the built-in table only")
    b = None
    if bias:
        b = get(f"{prefix}.bias")
        if tuple(b.shape) != (out_dim,):
            raise ValueError(f"shape mismatch for {prefix}.bias: expected [{out_dim}], got {list(b.shape)}")
    to = (lambda t: t) if device is None else (lambda t: None if t is None else t.to(device))
    return BnbLinear.from_parts(to(weight), to(absmax), quant_type, blocksize, shape, _DTYPES[state["dtype"]], to(b), to(nested_absmax), to(nested_quant_map),
                                nested_blocksize, nested_offset)
