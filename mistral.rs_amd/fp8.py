"""Host-side mirror of `FP8Linear` (mistralrs-quant/src/fp8/{mod,quantize}.rs: ISQ type F8E4M3, UQFF serde type 3) and `PerTensorFP8Linear`
(src/pertensor_fp8/: HF checkpoints with `quant_method: fp8` and `weight_block_size: null`) over the per-tensor FP8 kernels of csrc/fp8_pertensor.hip.

    q, s, dq = quantize_tensor(x)                                   # dynamic: s = min(448 / amax, 448), dq = 1 / s, q = fp8(x * s); all on the device
    q        = quantize_static(x, scale)                            # q = fp8(x / scale)
    w_hat    = dequantize(q, dq, torch.float32, ids=None)           # T(f32(q) * dq), optionally gathering rows
    y        = matmul_q(xq, wq, dq_x, dq_w, bias, torch.bfloat16)   # W8A8 on the FP8 matrix cores: RNE_T(fma(sum xq wq, dq_x * dq_w, bias))
    layer    = FP8Linear.quantize(w, bias)                          # the `--isq fp8` entry; layer.forward(x) quantizes x per call
    layer    = pertensor_fp8_linear_b(in_dim, out_dim, bias, tensors, prefix, act_quant="none")

E4M3 is OCP E4M3FN (bias 7, no infinities, 0x7f / 0xff NaN, max 448); `T -> fp8` is e4m3_satfinite_rne(f16_rne(clamp(f32(v), +-448))).  The arithmetic contract is
DESIGN 4.18; note there that the FP8 matrix core behind `matmul_q` (K % 16 == 0, aligned operands) does not add its products in f32: inside one instruction each
product is cut toward zero onto a grid 2^-13 of the instruction's largest one, and a row's bits may differ between an M = 16 and an M = 17 call.  PyTorch owns the buffers; every computation is a HIP kernel; nothing here synchronises with the host except the row-id check of a gather.  No CPU
fallback: apart from the loader's shape logic, tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import blockwise_fp8 as _bw
from .blockwise_fp8 import UnquantLinear, _as_bytes

FP8_E4M3_MAX = 448.0
ROUTES = {1: "mfma_gemv", 2: "mfma_tile", 3: "general"}
_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_TAG = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
_F8 = getattr(torch, "float8_e4m3fn", None)
UQFF_DTYPE_F8E4M3 = 9  # dtype_to_uqff_code (utils/uqff.rs:3-21)
HQQ_ISQ_GROUP_SIZE = 64  # ISQ_HQQ_GROUP_SIZE (lib.rs)


_FNS: dict = {}


def _fn(key: str, name: str, argtypes, restype=None):
    """A library entry point, resolved once."""
    f = _FNS.get(name)
    if f is None:
        f = _FNS[name] = _lib.sym(key, name, argtypes, restype)
    return f


def _state_floats() -> int:
    if "state" not in _FNS:
        _FNS["state"] = int(_lib.sym("quant", "fp8_pertensor_state_floats", [], C.c_int)())
    return _FNS["state"]


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("fp8: tensors must live on the GPU (no CPU fallback in this package)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rc(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def _src_code(x: torch.Tensor, what: str) -> int:
    if x.dtype not in _CODE:
        raise ValueError(f"Unsupported dtype for {what}: {x.dtype}")
    return _CODE[x.dtype]


def _scalar(scale: torch.Tensor, what: str) -> torch.Tensor:
    if scale.dtype == torch.float32 and scale.shape == (1,):
        return scale
    if scale.numel() != 1:
        raise ValueError(f"Expected {what} to be a scalar, got {list(scale.shape)}")
    return scale.to(torch.float32).reshape(1)


def fp8_pertensor_last_route() -> int:
    """Route code of the last per-tensor FP8 matmul launch (see ROUTES and csrc/fp8_pertensor.hip)."""
    return int(_fn("quant", "fp8_pertensor_last_route", [], C.c_int)())


def fp8_to_dtype(q: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """`scalar_fp8::ops::fp8_to_dtype`: exact, the NaN bytes give NaN."""
    q = _as_bytes(q).contiguous()
    _need_gpu(q)
    if dtype not in _TAG:
        raise ValueError(f"Unsupported dtype for fp8_to_dtype: {dtype}")
    out = torch.empty(q.shape, dtype=dtype, device=q.device)
    _fn("quant", f"launch_fp8_to_{_TAG[dtype]}_kernel", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])(q.data_ptr(), out.data_ptr(), q.numel(), _stream())
    return out


def dtype_to_fp8(x: torch.Tensor) -> torch.Tensor:
    """`scalar_fp8::ops::dtype_to_fp8`: e4m3_satfinite_rne(f16_rne(clamp(f32(v), +-448))) as u8 bytes."""
    _need_gpu(x)
    _src_code(x, "dtype_to_fp8")
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _fn("quant", f"launch_{_TAG[x.dtype]}_to_fp8_kernel", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])(x.data_ptr(), q.data_ptr(), x.numel(), _stream())
    return q


def quantize_tensor(x: torch.Tensor):
    """`FP8Linear::quantize` (fp8/quantize.rs:23-45) for f32 / f16 / bf16: (q u8 of x's shape, quantize scale s f32 [1], dequantize scale dq = 1 / s f32 [1]).
    amax, s and dq are computed and kept on the device; no host synchronisation."""
    _need_gpu(x)
    code = _src_code(x, "FP8 quantize")
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    state = torch.empty(_state_floats(), dtype=torch.float32, device=x.device)
    _rc(_fn("ext", "mrs_fp8_quantize_dynamic", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p], C.c_int)(
        x.data_ptr(), q.data_ptr(), x.numel(), state.data_ptr(), code, _stream()), "mrs_fp8_quantize_dynamic")
    return q, state[1:2], state[2:3]


def quantize_static(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """`fp8_pertensor_quantize` (pertensor_fp8/ops.rs:25-32): q = fp8(f32(x) / scale), scale a scalar on the device."""
    _need_gpu(x, scale)
    code = _src_code(x, "FP8 quantize")
    x, scale = x.contiguous(), _scalar(scale, "the activation scale")
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _rc(_fn("ext", "mrs_fp8_quantize_static", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p], C.c_int)(
        x.data_ptr(), q.data_ptr(), x.numel(), scale.data_ptr(), code, _stream()), "mrs_fp8_quantize_static")
    return q


def dequantize(w: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32, ids: torch.Tensor | None = None) -> torch.Tensor:
    """`fp8_pertensor_dequantize` / `FP8Linear::dequantize` / `embedding_forward_raw`: T(f32(w) * scale), bit exact.  With `ids` (any integer tensor) the rows
    ids of the rank-2 `w` are gathered: the result is ids.shape + [K].  A row id outside [0, N) is an error."""
    w = _as_bytes(w).contiguous()
    _need_gpu(w, scale, ids)
    if dtype not in _CODE:
        raise ValueError(f"Unsupported dtype for FP8 dequantize: {dtype}")
    scale = _scalar(scale, "the dequantize scale")
    fn = _fn("ext", "mrs_fp8_dequantize", [C.c_void_p] * 4 + [C.c_longlong, C.c_int, C.c_int, C.c_void_p], C.c_int)
    if ids is None:
        out = torch.empty(w.shape, dtype=dtype, device=w.device)
        _rc(fn(w.data_ptr(), scale.data_ptr(), None, out.data_ptr(), w.numel(), 1, _CODE[dtype], _stream()), "mrs_fp8_dequantize")
        return out
    if w.dim() != 2:
        raise ValueError(f"Expected a rank-2 weight for a row gather, got {list(w.shape)}")
    n, k = w.shape
    flat = ids.reshape(-1)
    if flat.numel():
        lo, hi = torch.stack(torch.aminmax(flat)).tolist()  # the one host read of a gather
        if lo < 0 or hi >= n:
            raise ValueError(f"embedding index {lo if lo < 0 else hi} is out of bounds for {n} rows")
    flat = flat.to(torch.int32).contiguous()
    out = torch.empty(*ids.shape, k, dtype=dtype, device=w.device)
    _rc(fn(w.data_ptr(), scale.data_ptr(), flat.data_ptr(), out.data_ptr(), flat.numel(), k, _CODE[dtype], _stream()), "mrs_fp8_dequantize")
    return out


def matmul_q(xq: torch.Tensor, wq: torch.Tensor, dq_x: torch.Tensor, dq_w: torch.Tensor, bias: torch.Tensor | None = None,
             dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """W8A8: xq [M, K] and wq [N, K] E4M3 bytes (contiguous views keep their address: an unaligned one takes the general route), dq_x / dq_w f32 scalars on
    the device, bias [N] -> [M, N] `dtype` (bf16 / f16) = RNE(fma(sum_k xq wq, dq_x * dq_w, bias))."""
    xq, wq = _as_bytes(xq), _as_bytes(wq)
    _need_gpu(xq, wq, dq_x, dq_w, bias)
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"Unsupported output dtype for the FP8 matmul: {dtype}")
    if xq.dim() != 2:
        raise ValueError(f"Expected input to be rank 2, got {list(xq.shape)}")
    m, k = xq.shape
    if wq.dim() != 2 or wq.shape[1] != k:
        raise ValueError(f"Weight shape mismatch: expected [N, K] = [N, {k}], got {list(wq.shape)}")
    n = wq.shape[0]
    if bias is not None and tuple(bias.shape) != (n,):
        raise ValueError(f"Bias shape mismatch: expected [{n}], got {list(bias.shape)}")
    xq, wq = xq.contiguous(), wq.contiguous()
    dq_x, dq_w = _scalar(dq_x, "dq_x"), _scalar(dq_w, "dq_w")
    bias = None if bias is None else bias.to(dtype).contiguous()
    out = torch.empty(m, n, dtype=dtype, device=xq.device)
    if m and n:
        if k == 0:
            raise ValueError("The FP8 matmul needs K > 0")
        _rc(_fn("ext", "mrs_fp8_matmul", [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p], C.c_int)(
            xq.data_ptr(), wq.data_ptr(), dq_x.data_ptr(), dq_w.data_ptr(), _ptr(bias), out.data_ptr(), m, n, k, _CODE[dtype], _stream()), "mrs_fp8_matmul")
    return out


def _isq_from_dense(weight: torch.Tensor, bias, dtype, imatrix_weight, who: str, targets=("HQQ", "MXFP4", "GGML")):
    """The dense-weight branches shared by the two layers' apply_isq: the quantizers BlockwiseFP8Linear.apply_isq hands its dequantized weight to."""
    from . import hqq, isq, mxfp4
    from .gguf.matmul import GgufMatMul
    from .gguf.qtensor import GgmlDType
    if dtype in ("HQQ4", "HQQ8"):
        if imatrix_weight is not None:
            raise ValueError("HQQ does not support imatrix.")
        cfg = hqq.HqqConfig(bits=int(dtype[3:]), group_size=HQQ_ISQ_GROUP_SIZE, axis=0, optimization_steps=hqq.OPTIMIZER_HQQ_DEFAULT_STEPS, round_zeros=False,
                            channel_wise=True)
        res = hqq.HqqLayer.quantize(weight, cfg)
        return res if bias is None else res.with_bias(bias.to(res.scales.dtype))
    if dtype == "MXFP4":
        if imatrix_weight is not None:
            raise ValueError("MXFP4 does not support imatrix.")
        return mxfp4.MXFP4Layer.quantize(weight, bias)
    if "AFQ" in targets and dtype in ("AFQ2", "AFQ3", "AFQ4", "AFQ6", "AFQ8"):
        from . import afq
        if imatrix_weight is not None:
            raise ValueError("AFQ does not support imatrix.")
        return afq.AfqLayer.quantize(weight, bias, bits=int(dtype[3:]))
    if dtype is None:
        return UnquantLinear(weight, bias)  # the imatrix is ignored altogether
    if isinstance(dtype, GgmlDType):
        target = isq.get_quantization_behaviour(weight.shape, dtype)
        if target is None:
            raise ValueError(f"isq: no GGML type fits a weight of shape {list(weight.shape)} for {dtype.name}")
        q = isq.quantize_imatrix(weight, imatrix_weight, target) if imatrix_weight is not None and isq.imatrix_capable(target) else isq.quantize(weight, target)
        return GgufMatMul(q, None if bias is None else bias.to(torch.float32))
    raise ValueError(f"{who} apply_isq: unsupported ISQ type {dtype!r}")


def _check_weight(weight, bias, who):
    weight = _as_bytes(weight)
    if weight.dim() != 2:
        raise ValueError(f"{who} weight must be [N, K], got {list(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"Bias shape mismatch: expected [{weight.shape[0]}], got {list(bias.shape)}")
    return weight


def _forward_q(x: torch.Tensor, weight, dq_w, bias, static_scale=None) -> torch.Tensor:
    """Flatten the leading dims, quantize x (dynamically, or by the static scale whose value is then also dq_x), W8A8 matmul, restore the dims."""
    if x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"Expected input [..., {weight.shape[1]}], got {list(x.shape)}")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"Unsupported dtype for the FP8 forward: {x.dtype}")
    x2 = x.reshape(-1, x.shape[-1])
    if static_scale is None:
        xq, _, dq_x = quantize_tensor(x2)
    else:
        xq, dq_x = quantize_static(x2, static_scale), static_scale
    return matmul_q(xq, weight, dq_x, dq_w, bias, x.dtype).reshape(*x.shape[:-1], weight.shape[0])


class FP8Linear:
    """fp8/mod.rs.  weight E4M3 bytes [N, K]; dequant_w_scale, dequant_x_scale, quant_scale f32 scalars (dequant_x_scale is the stored one of the reference: the
    forward quantizes x per call and uses that call's scale)."""

    def __init__(self, weight, bias, dequant_w_scale, dequant_x_scale, quant_scale):
        self.weight, self.bias = _check_weight(weight, bias, "FP8"), bias
        self.dequant_w_scale, self.dequant_x_scale, self.quant_scale = (_scalar(t, n) for t, n in (
            (dequant_w_scale, "dequant_w_scale"), (dequant_x_scale, "dequant_x_scale"), (quant_scale, "quant_scale")))

    @classmethod
    def from_parts(cls, weight, bias, dequant_w_scale, dequant_x_scale, quant_scale) -> "FP8Linear":
        return cls(weight, bias, dequant_w_scale, dequant_x_scale, quant_scale)

    @classmethod
    def quantize(cls, w: torch.Tensor, bias: torch.Tensor | None = None) -> "FP8Linear":
        """The ISQ `fp8` entry (mod.rs:138-151): dequant_x_scale starts as a copy of dequant_w_scale, as there."""
        if w.dim() != 2:
            raise ValueError(f"FP8 weight must be [N, K], got {list(w.shape)}")
        q, s, dq = quantize_tensor(w)
        return cls(q, bias, dq, dq.clone(), s)

    def has_bias(self) -> bool:
        return self.bias is not None

    def dtype_and_device(self):
        return (_F8 or "F8E4M3"), self.weight.device

    def quantized_act_type(self):
        return None

    def name(self) -> str:
        return "fp8-linear"

    def uqff_type(self) -> str:
        return "F8E4M3"

    def isq_serde_supported(self) -> bool:
        return True

    def dequantize(self, dtype: torch.dtype) -> torch.Tensor:
        return dequantize(self.weight, self.dequant_w_scale, dtype)

    def dequantize_w(self) -> torch.Tensor:
        return self.dequantize(torch.float32)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _forward_q(x, self.weight, self.dequant_w_scale, self.bias)

    def embedding_forward(self, ids: torch.Tensor) -> torch.Tensor:
        """mod.rs:158-171: gather, then f32 * dequant_w_scale; ids.shape + [K]."""
        return dequantize(self.weight, self.dequant_w_scale, torch.float32, ids)

    def add_delta_w(self, delta: torch.Tensor) -> "FP8Linear":
        return FP8Linear.quantize(self.dequantize(delta.dtype) + delta, self.bias)

    def apply_isq(self, dtype, imatrix_weight=None):
        """mod.rs:269-299."""
        if dtype is None or (dtype == "F8E4M3" and imatrix_weight is None):
            return self
        if dtype == "F8E4M3":
            raise ValueError("F8E4M3 does not support imatrix.")
        return _isq_from_dense(self.dequantize_w(), self.bias, dtype, imatrix_weight, "FP8")

    def serialize_uqff(self, prefix: str) -> dict:
        from . import uqff
        w = self.weight.cpu()
        return uqff.serialize_fp8_layer(prefix, w.view(_F8) if _F8 is not None else w, self.dequant_w_scale.cpu(), self.dequant_x_scale.cpu(), self.quant_scale.cpu(),
                                        None if self.bias is None else self.bias.cpu())


class PerTensorFP8Linear:
    """pertensor_fp8/mod.rs.  The E4M3 bytes stay resident (the reference dequantizes at load only because candle has no FP8 ops).  `act_quant`: "none" weight-only
    (the blockwise matmul with a 1 x 1 scale grid), "static" (activation_scale), "dynamic" (per call)."""

    def __init__(self, weight, weight_scale_inv, activation_scale=None, bias=None, dequant_dtype: torch.dtype = torch.bfloat16, act_quant: str = "none"):
        self.weight, self.bias = _check_weight(weight, bias, "Per-tensor FP8"), bias
        self.weight_scale_inv = _scalar(weight_scale_inv, "weight_scale_inv")
        self.activation_scale = None if activation_scale is None else _scalar(activation_scale, "activation_scale")
        if dequant_dtype not in _CODE:
            raise ValueError(f"Unsupported dequant_dtype for per-tensor FP8: {dequant_dtype}")
        if act_quant not in ("none", "static", "dynamic"):
            raise ValueError(f"Unknown act_quant {act_quant!r}; expected `none`, `static` or `dynamic`")
        if act_quant == "static" and activation_scale is None:
            raise ValueError("act_quant `static` needs an activation_scale")
        self.dequant_dtype, self.act_quant = dequant_dtype, act_quant

    def has_bias(self) -> bool:
        return self.bias is not None

    def dtype_and_device(self):
        return (_F8 or "F8E4M3"), self.weight.device

    def quantized_act_type(self):
        return None

    def name(self) -> str:
        return "pertensor-fp8-linear"

    def isq_serde_supported(self) -> bool:
        return False

    def dequantize_w(self) -> torch.Tensor:
        return dequantize(self.weight, self.weight_scale_inv, self.dequant_dtype)

    def add_delta_w(self, delta):
        raise ValueError("PerTensorFP8Linear does not support add_delta_w")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.act_quant == "none":
            n, k = self.weight.shape
            y = _bw.matmul(x.reshape(-1, x.shape[-1]), self.weight, self.weight_scale_inv.reshape(1, 1), (n, k)).reshape(*x.shape[:-1], n)
            return y if self.bias is None else y + self.bias.to(y.dtype)
        return _forward_q(x, self.weight, self.weight_scale_inv, self.bias, self.activation_scale if self.act_quant == "static" else None)

    def apply_isq(self, dtype, imatrix_weight=None):
        """mod.rs:103-259 (F8Q8, CPU-only in the reference, is not a target here)."""
        if dtype == "F8E4M3":
            if imatrix_weight is not None:
                raise ValueError("F8E4M3 does not support imatrix.")
            return FP8Linear.quantize(self.dequantize_w(), self.bias)
        return _isq_from_dense(self.dequantize_w(), self.bias, dtype, imatrix_weight, "Per-tensor FP8", targets=("HQQ", "MXFP4", "GGML", "AFQ"))


def pertensor_fp8_linear_b(in_dim: int, out_dim: int, bias: bool, tensors: dict, prefix: str, act_quant: str = "none", device=None):
    """mod.rs:278-335 over a dict of checkpoint tensors: a plain `weight` without `weight_scale_inv` is an UnquantLinear; the dequantize dtype is the bias's, else
    bf16; `activation_scale` and `bias` are optional tensors."""
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    has = lambda s: f"{prefix}.{s}" in tensors
    missing = [f"{prefix}.{s}" for s in ("weight", "weight_scale_inv") if not has(s)]
    if has("weight") and not has("weight_scale_inv"):
        w = _bw._get(tensors, f"{prefix}.weight", (out_dim, in_dim))
        return UnquantLinear(to(w), to(_bw._get(tensors, f"{prefix}.bias", (out_dim,))) if bias and has("bias") else None)
    if missing:
        raise ValueError(f"pertensor_fp8_linear: cannot find tensor {', '.join(missing)}")
    weight = _as_bytes(_bw._get(tensors, f"{prefix}.weight", (out_dim, in_dim)))
    scale = tensors[f"{prefix}.weight_scale_inv"]
    act = tensors[f"{prefix}.activation_scale"] if has("activation_scale") else None
    b = _bw._get(tensors, f"{prefix}.bias", (out_dim,)) if bias and has("bias") else None
    dd = b.dtype if b is not None and b.dtype in _CODE else torch.bfloat16
    return PerTensorFP8Linear(to(weight), to(scale), None if act is None else to(act), None if b is None else to(b), dd, act_quant)


def fp8_linear_from_uqff(reader, prefix: str, shard=None, device=None) -> FP8Linear:
    """`FP8Linear::from_uqff` (mod.rs:74-93) on a `uqff.UqffReader`."""
    d = reader.load_fp8_layer(prefix, shard)
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    return FP8Linear(to(_as_bytes(d.weight)), None if d.bias is None else to(d.bias), to(d.dequant_w_scale), to(d.dequant_x_scale), to(d.quant_scale))
