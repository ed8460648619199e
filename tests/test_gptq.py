"""CPU: GPTQ / AWQ -- a numpy oracle written from the format definition (pack / unpack along K and along N, the AWQ interleave, reconstruct; the GPU file
imports it), packer round trips with the 3-bit straddles, the un-wrapped zero point, the AWQ repack oracle against direct AWQ dequantization, the host
mirror's argument checks and error texts, the exported symbols, and the code objects of the GPTQ kernels (no scratch, no spills, the tile inside 256 VGPRs).
The oracle restates the format read from the reference's sources; it is not pinned to the reference's compiled kernels.  The GPU side is
tests/test_zz_gptq_gpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mistralrs_amd  # noqa: E402,F401
from mistralrs_amd import gptq  # noqa: E402

BITS = [2, 3, 4, 8]
GROUPS = [32, 64, 128]
AWQ_ORDER = {4: [0, 4, 1, 5, 2, 6, 3, 7], 8: [0, 2, 1, 3]}  # in-word position of logical column j


# ------------------------------------------------------------------------------------------------ oracle
def _pack_last(codes: np.ndarray, bits: int) -> np.ndarray:
    """codes [.., L] -> u32 [.., L * bits / 32]: element j in bits [j * bits, (j + 1) * bits) of the row's little-endian bit stream"""
    codes = np.asarray(codes, dtype=np.uint32)
    n = codes.shape[-1]
    assert (n * bits) % 32 == 0 and codes.max(initial=0) < (1 << bits)
    stream = ((codes[..., None] >> np.arange(bits, dtype=np.uint32)) & 1).astype(np.uint64).reshape(*codes.shape[:-1], n * bits // 32, 32)
    return (stream << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def _unpack_last(words: np.ndarray, bits: int) -> np.ndarray:
    words = np.asarray(words, dtype=np.uint32)
    stream = ((words[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(*words.shape[:-1], -1)
    n = stream.shape[-1] // bits
    return (stream.reshape(*words.shape[:-1], n, bits).astype(np.uint32) << np.arange(bits, dtype=np.uint32)).sum(-1).astype(np.uint32)


def pack_n(codes, bits):
    """codes [R, N] -> u32 [R, N * bits / 32], the bit stream along N (qzeros)"""
    return _pack_last(codes, bits)


def unpack_n(words, bits):
    return _unpack_last(words, bits)


def pack_k(codes, bits):
    """codes [K, N] -> u32 [K * bits / 32, N]: column n's K codes as one bit stream down the rows (GPTQ qweight)"""
    return np.ascontiguousarray(_pack_last(np.asarray(codes).T, bits).T)


def unpack_k(words, bits):
    return np.ascontiguousarray(_unpack_last(np.asarray(words).T, bits).T)


def awq_interleave(codes, bits):
    """logical codes [R, N] -> AWQ words [R, N * bits / 32]: logical column j of a word sits at in-word position AWQ_ORDER[bits][j]"""
    codes = np.asarray(codes, dtype=np.uint32)
    pack = 32 // bits
    c = codes.reshape(codes.shape[0], -1, pack)
    placed = np.zeros_like(c)
    placed[..., AWQ_ORDER[bits]] = c
    return _pack_last(placed.reshape(codes.shape), bits)


def awq_deinterleave(words, bits):
    pack = 32 // bits
    placed = _unpack_last(words, bits).reshape(words.shape[0], -1, pack)
    return placed[..., AWQ_ORDER[bits]].reshape(words.shape[0], -1)


def reconstruct(qweight, qzeros, scales, g_idx, bits, zero_offset):
    """f16 [K, N]: W[k][n] = f16_rne((q - (z + zero_offset)) * s), the integer exact in f16, the product ONE rounding (taken in f64: 9 + 11 bits, exact)"""
    q = unpack_k(qweight, bits).astype(np.int64)
    z = unpack_n(qzeros, bits).astype(np.int64)[np.asarray(g_idx)]
    s = np.asarray(scales, dtype=np.float16).astype(np.float64)[np.asarray(g_idx)]
    with np.errstate(over="ignore"):
        return ((q - z - zero_offset).astype(np.float64) * s).astype(np.float16)


def awq_dequantize(qweight_awq, qzeros_awq, scales, bits, group):
    """direct AWQ dequantization, no repack: W = f16_rne((q - z) * s), group = k // group_size"""
    q = awq_deinterleave(qweight_awq, bits).astype(np.int64)
    z = np.repeat(awq_deinterleave(qzeros_awq, bits).astype(np.int64), group, 0)
    s = np.repeat(np.asarray(scales, dtype=np.float16).astype(np.float64), group, 0)
    return ((q - z).astype(np.float64) * s).astype(np.float16)


def awq_repack(qweight_awq, qzeros_awq, bits, group):
    """the repack oracle: (qweight [K * bits / 32, N], qzeros [G, N * bits / 32], g_idx [K]) in GPTQ layout, zero offset 0"""
    k = qweight_awq.shape[0]
    return pack_k(awq_deinterleave(qweight_awq, bits), bits), pack_n(awq_deinterleave(qzeros_awq, bits), bits), (np.arange(k) // group).astype(np.int32)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


# ------------------------------------------------------------------------------------------------ oracle checks
def test_packers_round_trip_and_three_bit_straddles():
    rng = np.random.default_rng(0)
    for bits in BITS:
        codes = rng.integers(0, 1 << bits, (96, 64), dtype=np.uint32)
        wk = pack_k(codes, bits)
        assert wk.shape == (96 * bits // 32, 64) and np.array_equal(unpack_k(wk, bits), codes)
        wn = pack_n(codes, bits)
        assert wn.shape == (96, 64 * bits // 32) and np.array_equal(unpack_n(wn, bits), codes)
    # 2 / 4 / 8 bits: 32 / bits codes per word, code i of a word at bit i * bits
    for bits in (2, 4, 8):
        c = np.zeros((32, 32), np.uint32)
        c[1, 5] = 1
        assert pack_k(c, bits)[0, 5] == 1 << bits and pack_n(c.T, bits)[5, 0] == 1 << bits
    # 3 bits: 32 codes per 3 words; code 10 has its low 2 bits at the top of word 0 and its top bit at the bottom of word 1, code 21 its low bit at the
    # top of word 1 and its upper two bits at the bottom of word 2 -- what the reference's 3-bit kernel reassembles as (w1 >> 30) | ((w2 << 2) & 4) and
    # (w2 >> 31) | ((w3 << 1) & 6)
    c = np.zeros((32, 32), np.uint32)
    c[10, 7], c[21, 7] = 0b101, 0b110
    w = pack_k(c, 3)
    assert w.shape == (3, 32) and list(w[:, 7]) == [0b01 << 30, 0b1, 0b11] and not w[:, :7].any()
    w1, w2, w3 = (int(v) for v in w[:, 7])
    assert (w1 >> 30) | ((w2 << 2) & 4) == 0b101 and (w2 >> 31) | ((w3 << 1) & 6) == 0b110
    assert list(pack_n(c.T, 3)[7]) == [0b01 << 30, 0b1, 0b11]
    for bits in (4, 8):
        codes = rng.integers(0, 1 << bits, (5, 64), dtype=np.uint32)
        assert np.array_equal(awq_deinterleave(awq_interleave(codes, bits), bits), codes)
    # AWQ: logical column 1 of a 4-bit word sits in nibble 4, logical column 2 of an 8-bit word in byte 1
    c = np.zeros((1, 32), np.uint32)
    c[0, 1] = 0xA
    assert awq_interleave(c, 4)[0, 0] == 0xA << 16
    c = np.zeros((1, 32), np.uint32)
    c[0, 2] = 0xAB
    assert awq_interleave(c, 8)[0, 0] == 0xAB << 8


@pytest.mark.parametrize("bits", BITS)
def test_stored_zero_is_not_wrapped(bits):
    top = (1 << bits) - 1
    k, n = max(32, top + 1), 32  # every code once
    codes = np.tile(np.arange(k, dtype=np.uint32)[:, None] % (top + 1), (1, n))
    zeros = np.full((1, n), top, np.uint32)
    zeros[0, 1] = 0
    scales = np.full((1, n), 0.5, np.float16)
    w = reconstruct(pack_k(codes, bits), pack_n(zeros, bits), scales, np.zeros(k, np.int32), bits, 1)
    # stored 2^bits - 1 means 2^bits: code 0 -> -2^bits * s, the top code -> -1 * s (a wrapped zero of 0 would give 0 and top * s)
    assert float(w[0, 0]) == -(top + 1) * 0.5 and float(w[top, 0]) == -0.5
    assert float(w[0, 1]) == -0.5 and float(w[top, 1]) == (top - 1) * 0.5
    # the AWQ offset: a true zero point of 0 is representable
    w0 = reconstruct(pack_k(codes, bits), pack_n(zeros, bits), scales, np.zeros(k, np.int32), bits, 0)
    assert float(w0[0, 1]) == 0.0 and float(w0[top, 1]) == top * 0.5 and float(w0[0, 0]) == -top * 0.5


@pytest.mark.parametrize("bits", [4, 8])
def test_awq_repack_oracle_equals_direct_dequantization(bits):
    rng = np.random.default_rng(bits)
    for group, k, n in [(32, 96, 64), (64, 128, 32), (128, 128, 96)]:
        codes = rng.integers(0, 1 << bits, (k, n), dtype=np.uint32)
        zeros = rng.integers(0, 1 << bits, (k // group, n), dtype=np.uint32)
        zeros[0, :3] = [0, (1 << bits) - 1, 1]
        scales = (rng.uniform(0.5, 2.0, (k // group, n)) * 2.0 ** rng.integers(-8, -3, (k // group, n))).astype(np.float16)
        qw_a, qz_a = awq_interleave(codes, bits), awq_interleave(zeros, bits)
        direct = awq_dequantize(qw_a, qz_a, scales, bits, group)
        qw, qz, gi = awq_repack(qw_a, qz_a, bits, group)
        assert qw.shape == (k * bits // 32, n) and qz.shape == (k // group, n * bits // 32) and np.array_equal(gi, np.arange(k) // group)
        assert np.array_equal(unpack_k(qw, bits), codes) and np.array_equal(unpack_n(qz, bits), zeros)
        assert np.array_equal(reconstruct(qw, qz, scales, gi, bits, 0).view(np.uint16), direct.view(np.uint16))


# ------------------------------------------------------------------------------------------------ host mirror
def _parts(bits=4, group=32, k=64, n=32, seed=0):
    rng = np.random.default_rng(seed)
    g = k // group
    qweight = i32(pack_k(rng.integers(0, 1 << bits, (k, n), dtype=np.uint32), bits))
    qzeros = i32(pack_n(rng.integers(0, 1 << bits, (g, n), dtype=np.uint32), bits))
    scales = torch.from_numpy(rng.uniform(0.01, 0.1, (g, n)).astype(np.float16))
    g_idx = torch.from_numpy((np.arange(k) // group).astype(np.int32))
    return qweight, qzeros, scales, g_idx


def test_layer_surface_and_argument_errors():
    qw, qz, sc, gi = _parts()
    bias = torch.zeros(32, dtype=torch.float16)
    layer = gptq.GptqLayer.from_parts(qw, qz, sc, gi, bias, 4)
    assert layer.name() == "gptq" and layer.has_bias() and not layer.isq_serde_supported() and layer.quantized_act_type() == torch.float16
    assert layer.dtype_and_device() == (torch.float16, sc.device) and not layer.is_awq and layer.zero_offset == 1
    assert (layer.in_features, layer.out_features, layer.groups, layer.group_size) == (64, 32, 2, 32)
    assert gptq.ROUTES == {1: "gemv", 2: "mfma_tile"}
    with pytest.raises(ValueError, match="GPTQ quantization does not support ISQ."):
        layer.apply_isq("Q4K")
    with pytest.raises(ValueError, match="GPTQ quantization does not support adding weight delta."):
        layer.add_delta_w(torch.zeros(32, 64))
    with pytest.raises(ValueError, match="gptq does not support `gather_forward`. Please raise an issue."):
        layer.gather_forward(torch.zeros(1, 64), torch.zeros(1, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="must live on the GPU"):
        layer.forward(torch.zeros(1, 64))
    with pytest.raises(ValueError, match="must live on the GPU"):
        layer.dequantize_w()
    with pytest.raises(ValueError, match="forward_raw expects f16 activations, got torch.bfloat16"):
        layer.forward_raw(torch.zeros(1, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r"expects x \[..., K = 64\]"):
        layer.forward_raw(torch.zeros(1, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="Invalid GPTQ bits 6."):
        gptq.GptqLayer.from_parts(qw, qz, sc, gi, None, 6)
    with pytest.raises(ValueError, match="Invalid AWQ bits 3."):
        gptq.GptqLayer.from_parts(qw, qz, sc, None, None, 3, is_awq=True)
    with pytest.raises(ValueError, match="GPTQ needs g_idx"):
        gptq.GptqLayer.from_parts(qw, qz, sc, None, None, 4)
    with pytest.raises(ValueError, match="Bias mismatch"):
        gptq.GptqLayer.from_parts(qw, qz, sc, gi, bias.float(), 4)
    # the AWQ repack is a kernel: CPU parts stop at the guard, after the shape rules
    with pytest.raises(ValueError, match="must live on the GPU"):
        gptq.GptqLayer.from_parts(torch.zeros(64, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), sc, None, None, 4, is_awq=True)
    with pytest.raises(ValueError, match="AWQ qzeros have G = 2 groups, expected K / group_size = 1"):
        gptq.awq_repack(torch.zeros(64, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), 4, 64)


def test_shape_rules_name_the_dimension():
    qw, qz, sc, gi = _parts()
    with pytest.raises(ValueError, match="in_features K = 16 must be a multiple of 32"):
        gptq.check_parts(qw[:2], qz[:1], sc[:1], gi[:16], 4)
    with pytest.raises(ValueError, match="out_features N = 16 must be a multiple of 32"):
        gptq.check_parts(qw[:, :16].contiguous(), qz[:, :2].contiguous(), sc[:, :16].contiguous(), gi, 4)
    with pytest.raises(ValueError, match="in_features K = 64 must be a multiple of group_size = 48"):
        gptq.check_parts(qw, qz, sc, gi, 4, 48)
    with pytest.raises(ValueError, match="scales have G = 2 groups, expected K / group_size = 1"):
        gptq.check_parts(qw, qz, sc, gi, 4, 64)
    with pytest.raises(ValueError, match=r"qzeros must be \[G, N \* bits / 32\] = \[2, 4\]"):
        gptq.check_parts(qw, qz[:, :2].contiguous(), sc, gi, 4)
    with pytest.raises(ValueError, match="g_idx must have K = 64 entries, got 32"):
        gptq.check_parts(qw, qz, sc, gi[:32], 4)
    bad = gi.clone()
    bad[5] = 2
    with pytest.raises(ValueError, match=r"g_idx value 2 is outside \[0, G = 2\)"):
        gptq.GptqLayer.from_parts(qw, qz, sc, bad, None, 4)
    bad[5] = -1
    with pytest.raises(ValueError, match=r"g_idx value -1 is outside \[0, G = 2\)"):
        gptq.GptqLayer.from_parts(qw, qz, sc, bad, None, 4)
    with pytest.raises(ValueError, match="scales must be f16"):
        gptq.check_parts(qw, qz, sc.float(), gi, 4)
    with pytest.raises(ValueError, match="must be i32"):
        gptq.check_parts(qw.float(), qz, sc, gi, 4)
    assert gptq.check_parts(qw, qz, sc, gi, 4) == (64, 32, 2)
    q3 = _parts(bits=3)
    assert gptq.check_parts(*q3, 3) == (64, 32, 2) and tuple(q3[0].shape) == (6, 32) and tuple(q3[1].shape) == (2, 3)


def test_gptq_linear_loader():
    qw, qz, sc, gi = _parts()
    bias = torch.zeros(32, dtype=torch.float16)
    cfg = {"quant_method": "gptq", "bits": 4, "group_size": 32}
    tensors = {"p.qweight": qw, "p.qzeros": qz, "p.scales": sc, "p.g_idx": gi}
    layer = gptq.gptq_linear(64, 32, cfg, tensors, "p")
    assert isinstance(layer, gptq.GptqLayer) and not layer.has_bias() and layer.bits == 4 and layer.group_size == 32 and not layer.is_awq
    assert gptq.gptq_linear(64, 32, {**cfg, "checkpoint_format": "gptq"}, {**tensors, "p.bias": bias}, "p").has_bias()
    with pytest.raises(ValueError, match="checkpoint_format 'marlin' is not supported"):
        gptq.gptq_linear(64, 32, {**cfg, "checkpoint_format": "marlin"}, tensors, "p")
    for bad in ({"quant_method": "fp8", "bits": 4, "group_size": 32}, {"quant_method": "gptq", "bits": 4}, {"bits": 4, "group_size": 32}, None):
        with pytest.raises(ValueError, match="Unexpected quantization config."):
            gptq.gptq_linear(64, 32, bad, tensors, "p")
    with pytest.raises(ValueError, match="cannot find tensor p.g_idx"):
        gptq.gptq_linear(64, 32, cfg, {k: v for k, v in tensors.items() if k != "p.g_idx"}, "p")
    with pytest.raises(ValueError, match="cannot find tensor q.qweight"):
        gptq.gptq_linear(64, 32, cfg, tensors, "q")
    with pytest.raises(ValueError, match=r"shape mismatch for p.qweight: expected \[8, 64\], got \[8, 32\]"):
        gptq.gptq_linear(64, 64, cfg, tensors, "p")
    with pytest.raises(ValueError, match=r"shape mismatch for p.qzeros: expected \[1, 4\], got \[2, 4\]"):
        gptq.gptq_linear(64, 32, {**cfg, "group_size": 64}, tensors, "p")
    with pytest.raises(ValueError, match="dtype mismatch for p.scales"):
        gptq.gptq_linear(64, 32, cfg, {**tensors, "p.scales": sc.float()}, "p")
    with pytest.raises(ValueError, match="dtype mismatch for p.bias"):
        gptq.gptq_linear(64, 32, cfg, {**tensors, "p.bias": bias.float()}, "p")
    with pytest.raises(ValueError, match="must be a multiple of group_size = 48"):
        gptq.gptq_linear(64, 32, {**cfg, "group_size": 48}, tensors, "p")
    with pytest.raises(ValueError, match="Invalid AWQ bits 2."):
        gptq.gptq_linear(64, 32, {"quant_method": "awq", "bits": 2, "group_size": 32}, tensors, "p")
    # AWQ: the qweight is [in, out * bits / 32] and needs no g_idx; the repack itself is a kernel
    awq = {"p.qweight": torch.zeros(64, 4, dtype=torch.int32), "p.qzeros": qz, "p.scales": sc}
    with pytest.raises(ValueError, match="must live on the GPU"):
        gptq.gptq_linear(64, 32, {"quant_method": "awq", "bits": 4, "group_size": 32}, awq, "p")
    with pytest.raises(ValueError, match=r"shape mismatch for p.qweight: expected \[64, 4\], got \[8, 32\]"):
        gptq.gptq_linear(64, 32, {"quant_method": "awq", "bits": 4, "group_size": 32}, tensors, "p")
    # a plain weight under the prefix: the unquantized layer, without a bias
    plain = gptq.gptq_linear(64, 32, cfg, {"p.weight": torch.zeros(32, 64, dtype=torch.float16), "p.bias": bias}, "p")
    assert plain.name() == "unquant-linear" and not plain.has_bias()
    # the FP8 loader still refuses a gptq config
    from mistralrs_amd import blockwise_fp8
    with pytest.raises(ValueError, match="Unexpected quantization config."):
        blockwise_fp8.blockwise_fp8_module_kind(cfg, ["p.weight"], "p")


# ------------------------------------------------------------------------------------------------ the built libraries
NEW_SYMBOLS = {
    "libmistralrsquant.so": ["reconstruct_gptq", "gemm_half_q_half_alt", "launch_gptq_matmul", "launch_gptq_reconstruct", "launch_awq_repack", "gptq_last_route"],
    "libmrs_hip_ext.so": ["mrs_gptq_matmul", "mrs_gptq_reconstruct", "mrs_awq_repack"],
}


@pytest.mark.parametrize("lib", sorted(NEW_SYMBOLS))
def test_new_symbols_are_declared_and_exported(lib):
    path = os.path.join(ROOT, "mistral.rs_amd", "lib", lib)
    assert os.path.exists(path), f"{lib} is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "mistralrs_quant.h" if lib == "libmistralrsquant.so" else "mrs_hip_ext.h")).read()
    for name in NEW_SYMBOLS[lib]:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in the header"
        assert name in exported, f"{name} is not exported by {lib}"
    quant_header = open(os.path.join(ROOT, "include", "mistralrs_quant.h")).read()
    for name in ("reconstruct_exllama", "gemm_half_q_half_cuda_part"):  # named in the comment, never declared
        assert not re.search(r"\b" + name + r"\s*\(", quant_header)


def test_gptq_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    path = os.path.join(ROOT, "mistral.rs_amd", "lib", "libmistralrsquant.so")
    assert os.path.exists(path), "libmistralrsquant.so is not built"
    ks = [k for k in kernel_resources.resources(path) if re.search(r"gptq_|awq_", k.get("demangled", k["name"]))]
    gemv = [k for k in ks if "gptq_gemv_kernel" in k["demangled"]]
    tile = [k for k in ks if "gptq_tile_kernel" in k["demangled"]]
    assert len(gemv) == 16 and len(tile) == 4, (len(gemv), len(tile))  # 4 widths x 4 row counts; 4 widths
    assert any("gptq_reconstruct_kernel" in k["demangled"] for k in ks) and any("awq_repack_kernel" in k["demangled"] for k in ks)
    bad = [(k["demangled"], k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0), k.get("sgpr_spill_count", 0)) for k in ks
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0) or k.get("uses_dynamic_stack", False) is True]
    assert not bad, f"gptq kernels with scratch or spills: {bad}"
    over = [(k["demangled"], k.get("vgpr_count", 0)) for k in tile if k.get("vgpr_count", 0) > 256]
    assert not over, f"gptq tile kernels over 256 VGPRs: {over}"
    # static LDS inside the 64 KiB a kernel may declare
    lds = [(k["demangled"], k.get("group_segment_fixed_size", 0)) for k in ks if k.get("group_segment_fixed_size", 0) > 64 * 1024]
    assert not lds, lds
