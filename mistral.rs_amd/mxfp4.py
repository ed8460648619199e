"""Host-side mirror of `MXFP4Layer` (mistralrs-quant/src/mxfp4/mod.rs, ops.rs) over the drop-in MXFP4 C ABI of libmistralrsquant.so
(`launch_mxfp4_matmul_*`, `launch_mxfp4_indexed_moe_gemm_*`, `launch_mxfp4_moe_grouped_gemm_*`) and the row dequantizer of libmrs_hip_ext.so.

    layer = MXFP4Layer.quantize(w, bias)                  # [N, K] -> blocks u8 [N, K/2] + E8M0 scales u8 [N, K/32]
    layer = MXFP4Layer.from_parts(blocks, scales, bias)   # rank 2, or rank 3 for stacked experts [E, N, K/2]
    y     = layer.forward(x)                              # x [..., K] f16 / bf16 -> [..., N]
    y     = layer.gather_forward(x, indices)              # x [T, K] or [T, topk, K], indices [T, topk] -> [T, topk, N]
    w_hat = layer.dequantize_w()                          # bf16, the reference's dtype for this layer
    rows  = layer.embedding_forward(ids)                  # dequantized rows ids

Format: a byte holds two E2M1 values (low nibble = element k, high nibble = k + 1; magnitudes {0, .5, 1, 1.5, 2, 3, 4, 6}, bit 3 = sign); one E8M0 byte
scales 32 consecutive k and means f32_from_bits(s << 23).  PyTorch owns the buffers and runs the quantizer's elementwise algebra (load-time work); the
matmuls, the MoE gather and the dequantizer are the HIP kernels.  No CPU fallback: apart from `quantize` and the UQFF byte handling, tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

MXFP4_BLOCK_SIZE = 32  # mod.rs:20
FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_THRESHOLDS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)  # quantize_to_fp4 (mod.rs:427-457): a value on a boundary takes the upper nibble
_TAG = {torch.float16: "f16", torch.bfloat16: "bf16"}
_DEQ_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ROUTES = {1: "gemv", 2: "mfma_tile", 3: "moe_per_slot", 4: "moe_grouped_tile", 5: "gemv_chunks"}

_MATMUL_ARGS = [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_bool, C.c_void_p]
_MOE_ARGS = [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_bool, C.c_bool, C.c_void_p]


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("mxfp4: tensors must live on the GPU (no CPU fallback in this package)")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def last_route() -> int:
    """Route code of the last MXFP4 launch (see ROUTES and csrc/mxfp4.hip)."""
    return int(_lib.sym("quant", "mxfp4_last_route", [], C.c_int)())


def max_smem_optin() -> int:
    return int(_lib.sym("quant", "mxfp4_get_max_smem_optin", [], C.c_int)())


def _ptr(t):
    return None if t is None else t.data_ptr()


def dequantize_rows(blocks: torch.Tensor, scales: torch.Tensor, ids: torch.Tensor | None = None, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """blocks [R, K/2] / scales [R, K/32] -> [len(ids) or R, K]: row r is the dequantized row ids[r] (or r), converted once from the exact f32 value."""
    _need_gpu(blocks, scales, ids)
    if blocks.dim() != 2 or scales.dim() != 2 or blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError(f"mxfp4: expected rank-2 u8 blocks and scales, got {tuple(blocks.shape)} {blocks.dtype} and {tuple(scales.shape)} {scales.dtype}")
    if dtype not in _DEQ_CODE:
        raise ValueError(f"Unsupported dtype for MXFP4 dequantize: {dtype}")
    r, kh = blocks.shape
    k = kh * 2
    if k % MXFP4_BLOCK_SIZE or tuple(scales.shape) != (r, k // MXFP4_BLOCK_SIZE):
        raise ValueError(f"Scale shape mismatch: expected [N, K/32] = [{r}, {k // MXFP4_BLOCK_SIZE}], got {list(scales.shape)}")
    blocks, scales = blocks.contiguous(), scales.contiguous()
    if ids is not None:
        ids = ids.reshape(-1).to(torch.int32).contiguous()
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= r):
            raise ValueError(f"mxfp4: embedding ids must lie in 0..{r - 1}")
    rows = r if ids is None else ids.numel()
    out = torch.empty(rows, k, dtype=dtype, device=blocks.device)
    fn = _lib.sym("ext", "mrs_mxfp4_dequantize_rows", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p], C.c_int)
    rc = fn(blocks.data_ptr(), scales.data_ptr(), _ptr(ids), rows, k, _DEQ_CODE[dtype], out.data_ptr(), _stream())
    if rc != 0:
        raise RuntimeError(f"mrs_mxfp4_dequantize_rows failed ({rc})")
    return out


def matmul(x: torch.Tensor, blocks: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """`mxfp4_matmul` (ops.rs:16-214): x [M, K] f16 / bf16, blocks [N, K/2], scales [N, K/32], bias [N] -> [M, N]."""
    _need_gpu(x, blocks, scales, bias)
    if x.dim() != 2:
        raise ValueError(f"Expected input to be rank 2, got {list(x.shape)}")
    if x.dtype not in _TAG:
        raise ValueError(f"Unsupported dtype for MXFP4 matmul: {x.dtype}")
    m, k = x.shape
    n = blocks.shape[0]
    if blocks.dim() != 2 or blocks.shape[1] != k // 2 or k % MXFP4_BLOCK_SIZE:
        raise ValueError(f"Weight shape mismatch: expected [N, K/2] = [{n}, {k // 2}], got {list(blocks.shape)}")
    if tuple(scales.shape) != (n, k // MXFP4_BLOCK_SIZE):
        raise ValueError(f"Scale shape mismatch: expected [N, K/32] = [{n}, {k // MXFP4_BLOCK_SIZE}], got {list(scales.shape)}")
    x, blocks, scales = x.contiguous(), blocks.contiguous(), scales.contiguous()
    if bias is not None:
        if bias.numel() != n:
            raise ValueError(f"Bias shape mismatch: expected [{n}], got {list(bias.shape)}")
        bias = bias.to(x.dtype).contiguous()
    out = torch.empty(m, n, dtype=x.dtype, device=x.device)
    if m:
        _lib.sym("quant", f"launch_mxfp4_matmul_{_TAG[x.dtype]}", _MATMUL_ARGS)(
            x.data_ptr(), blocks.data_ptr(), scales.data_ptr(), _ptr(bias), out.data_ptr(), m, n, k, bias is not None, _stream())
    return out


def indexed_moe_gemm(x: torch.Tensor, blocks: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor | None, indices: torch.Tensor,
                     out: torch.Tensor | None = None, entry: str | None = None) -> torch.Tensor:
    """`mxfp4_indexed_moe_gemm` (ops.rs:313-614): x [T, K] or [T, topk, K], blocks [E, N, K/2], scales [E, N, K/32], bias [E, N], indices [T, topk] ->
    [T, topk, N].  `entry` picks the C symbol ("indexed" / "grouped"; default: the reference's rule, grouped when T > 1); both compute the same.  Rows whose
    expert id is >= E keep what `out` held (zeros when `out` is not given, as the reference's alloc_zeros)."""
    _need_gpu(x, blocks, scales, bias, indices)
    if x.dim() == 2:
        t, topk, k, has_topk = x.shape[0], indices.shape[-1], x.shape[1], False
    elif x.dim() == 3:
        t, topk, k, has_topk = x.shape[0], x.shape[1], x.shape[2], True
    else:
        raise ValueError(f"Expected input to be rank 2 or 3, got {list(x.shape)}")
    if x.dtype not in _TAG:
        raise ValueError(f"Unsupported dtype for MXFP4 indexed MoE GEMM: {x.dtype}")
    if blocks.dim() != 3 or blocks.shape[2] != k // 2 or k % MXFP4_BLOCK_SIZE:
        raise ValueError(f"Weight shape mismatch: expected [num_experts, N, K/2], got {list(blocks.shape)}")
    e, n = blocks.shape[0], blocks.shape[1]
    if tuple(scales.shape) != (e, n, k // MXFP4_BLOCK_SIZE):
        raise ValueError(f"Scale shape mismatch: expected [num_experts, N, K/32], got {list(scales.shape)}")
    if indices.numel() != t * topk:
        raise ValueError(f"Indices shape mismatch: expected [{t}, {topk}], got {list(indices.shape)}")
    x, blocks, scales = x.contiguous(), blocks.contiguous(), scales.contiguous()
    idx = indices.reshape(t, topk).to(torch.int64).to(torch.int32).contiguous()  # u32 ids: the same 32 bits
    if bias is not None:
        if tuple(bias.shape) != (e, n):
            raise ValueError(f"Bias shape mismatch: expected [{e}, {n}], got {list(bias.shape)}")
        bias = bias.to(x.dtype).contiguous()
    if out is None:
        out = torch.zeros(t, topk, n, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (t, topk, n) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError(f"mxfp4: `out` must be a contiguous {x.dtype} tensor of shape [{t}, {topk}, {n}]")
    entry = entry or ("grouped" if t > 1 else "indexed")
    name = {"indexed": "launch_mxfp4_indexed_moe_gemm_", "grouped": "launch_mxfp4_moe_grouped_gemm_"}[entry] + _TAG[x.dtype]
    if t:
        _lib.sym("quant", name, _MOE_ARGS)(x.data_ptr(), blocks.data_ptr(), scales.data_ptr(), _ptr(bias), idx.data_ptr(), out.data_ptr(), t, topk, e, n, k,
                                           bias is not None, has_topk, _stream())
    return out


def packed_gptoss_blocks(blocks_4d: torch.Tensor) -> torch.Tensor:
    """`packed_gptoss_linear` (mod.rs:550-567): GPT-OSS stores `*_blocks` as [E, N, K/32, 16]; the kernels read [E, N, K/2]."""
    if blocks_4d.dim() != 4 or blocks_4d.shape[-1] != MXFP4_BLOCK_SIZE // 2:
        raise ValueError(f"Expected GPT-OSS blocks of shape [num_experts, out_dim, num_blocks, 16], got {list(blocks_4d.shape)}")
    e, n, nb, _ = blocks_4d.shape
    return blocks_4d.reshape(e, n, nb * 16)


def quantize_tensors(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The quantizer of `MXFP4Layer::quantize` (mod.rs:340-457) in torch ops on w's device: per block of 32, scale byte = clamp(floor(log2(max|block| / 6)) + 127,
    0, 254) (127 for an all-zero block), every value times 2^(127 - scale) to the nearest E2M1 magnitude with boundary values going up, sign in bit 3 for values
    < 0, low nibble = even k.  floor(log2(.)) is taken exactly from the f32 exponent."""
    if w.dim() != 2:
        raise ValueError(f"MXFP4 quantization expects a rank-2 weight, got {list(w.shape)}")
    n, k = w.shape
    if k % MXFP4_BLOCK_SIZE:
        raise ValueError(f"MXFP4 quantization requires K ({k}) divisible by block size ({MXFP4_BLOCK_SIZE})")
    wf = w.detach().to(torch.float32).reshape(n, k // MXFP4_BLOCK_SIZE, MXFP4_BLOCK_SIZE)
    max_abs = wf.abs().amax(-1)
    _, ex = torch.frexp(max_abs / 6.0)                       # v = m * 2^ex, m in [.5, 1): floor(log2 v) = ex - 1
    scale = torch.where(max_abs == 0, torch.full_like(ex, 127), (ex - 1 + 127).clamp(0, 254)).to(torch.int32)
    inv = torch.ldexp(torch.ones_like(max_abs), 127 - scale)  # 1 / 2^(scale - 127), a power of two: the product below is exact
    v = wf * inv.unsqueeze(-1)
    a = v.abs()
    nib = torch.zeros_like(a, dtype=torch.int32)
    for t in _THRESHOLDS:
        nib += (a >= t).to(torch.int32)
    nib |= (v < 0).to(torch.int32) << 3
    nib = nib.reshape(n, k // 2, 2)
    blocks = (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8)
    return blocks.contiguous(), scale.to(torch.uint8).contiguous()


class MXFP4Layer:
    def __init__(self, blocks: torch.Tensor, scales: torch.Tensor, bias: torch.Tensor | None = None):
        if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise ValueError(f"MXFP4 blocks and scales must be u8 tensors, got {blocks.dtype} and {scales.dtype}")
        if blocks.dim() not in (2, 3) or scales.dim() != blocks.dim():
            raise ValueError(f"MXFP4 blocks must be [N, K/2] or [num_experts, N, K/2] with scales of the same rank, got {list(blocks.shape)} and {list(scales.shape)}")
        k = blocks.shape[-1] * 2
        if k % MXFP4_BLOCK_SIZE or tuple(scales.shape) != (*blocks.shape[:-1], k // MXFP4_BLOCK_SIZE):
            raise ValueError(f"Scale shape mismatch: expected {[*blocks.shape[:-1], k // MXFP4_BLOCK_SIZE]}, got {list(scales.shape)}")
        if bias is not None and tuple(bias.shape) != tuple(blocks.shape[:-1]):
            raise ValueError(f"Bias shape mismatch: expected {list(blocks.shape[:-1])}, got {list(bias.shape)}")
        self.blocks, self.scales, self.bias = blocks, scales, bias

    @classmethod
    def from_parts(cls, blocks, scales, bias=None) -> "MXFP4Layer":
        return cls(blocks, scales, bias)

    @classmethod
    def quantize(cls, w: torch.Tensor, bias: torch.Tensor | None = None) -> "MXFP4Layer":
        blocks, scales = quantize_tensors(w)
        return cls(blocks, scales, bias)

    # ---- QuantMethod surface
    def has_bias(self) -> bool:
        return self.bias is not None

    def dtype_and_device(self):
        return torch.bfloat16, self.scales.device  # mod.rs:192-194

    def uqff_type(self) -> str:
        return "MXFP4"

    @property
    def in_features(self) -> int:
        return self.blocks.shape[-1] * 2

    def dequantize_w(self, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        k = self.in_features
        flat = dequantize_rows(self.blocks.reshape(-1, k // 2), self.scales.reshape(-1, k // MXFP4_BLOCK_SIZE), None, dtype)
        return flat.reshape(*self.blocks.shape[:-1], k)

    def embedding_forward(self, ids: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
        if self.blocks.dim() != 2:
            raise ValueError(f"MXFP4 embedding expects rank-2 blocks, got {list(self.blocks.shape)}")
        rows = dequantize_rows(self.blocks, self.scales, ids.to(self.blocks.device), dtype)
        return rows.reshape(*ids.shape, self.in_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """`forward_raw` (mod.rs:106-126): leading dims are flattened for the matmul and restored."""
        if self.blocks.dim() != 2:
            raise ValueError(f"MXFP4 forward expects rank-2 blocks, got {list(self.blocks.shape)}; stacked experts go through gather_forward")
        if x.dim() < 2:
            raise ValueError(f"Expected input to be rank 2, got {list(x.shape)}")
        y = matmul(x.reshape(-1, x.shape[-1]), self.blocks, self.scales, self.bias)
        return y.reshape(*x.shape[:-1], y.shape[1])

    def gather_forward(self, x: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
        """`gather_forward_raw` (mod.rs:156-166)."""
        if self.blocks.dim() != 3:
            raise ValueError(f"Weight shape mismatch: expected [num_experts, N, K/2], got {list(self.blocks.shape)}")
        return indexed_moe_gemm(x, self.blocks, self.scales, self.bias, indices)

    # ---- UQFF (mod.rs:296-323,891-929)
    def serialize_uqff(self, prefix: str) -> dict:
        from . import uqff
        cpu = lambda t: None if t is None else t.detach().cpu().contiguous()
        return uqff.serialize_mxfp4_layer(prefix, cpu(self.blocks), cpu(self.scales), cpu(self.bias))

    @classmethod
    def from_uqff(cls, reader, prefix: str, device, shard=None) -> "MXFP4Layer":
        d = reader.load_mxfp4_layer(prefix, shard)
        to = lambda t: None if t is None else t.to(device)
        return cls(to(d.blocks), to(d.scales), to(d.bias))
