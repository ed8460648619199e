"""CPU: the per-tensor FP8 host mirror (mistralrs_amd.fp8) -- the numpy oracle of the quantizer chain that the GPU test uses, the UQFF type-3 round
trip, the loader's branches, the apply_isq identities and error texts, and the code objects of the kernels (no scratch, no spills).  The GPU side is
tests/test_zz_fp8_gpu.py."""
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mistralrs_amd  # noqa: E402,F401
from mistralrs_amd import fp8, uqff  # noqa: E402
from mistralrs_amd.blockwise_fp8 import UnquantLinear  # noqa: E402
from mistralrs_amd.distributed import Shard  # noqa: E402
from tests.test_blockwise_fp8 import e4m3_decode, e4m3_encode_f16  # noqa: E402

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the numpy oracle (shared with the GPU test)
def encode(v) -> np.ndarray:
    """T -> fp8 of the contract on f32 values: e4m3_satfinite_rne(f16_rne(clamp(v, +-448)))."""
    return e4m3_encode_f16(np.clip(np.asarray(v, dtype=F32), F32(-448.0), F32(448.0)).astype(np.float16))


def quant_dynamic_oracle(x):
    """FP8Linear::quantize on f32 values: (q, s, dq), s = min(448 / amax, 448) and dq = 1 / s in correctly rounded f32, q = fp8(x * s), one f32 product."""
    x = np.asarray(x, dtype=F32)
    amax = F32(np.max(np.abs(x))) if x.size else F32(0.0)
    with np.errstate(divide="ignore", over="ignore"):
        s = np.minimum(F32(448.0) / amax, F32(448.0)).astype(F32)
    return encode(x * s), s, (F32(1.0) / s).astype(F32)


def quant_static_oracle(x, scale):
    return encode(np.asarray(x, dtype=F32) / F32(scale))


def test_quantizer_oracle_on_hand_picked_values():
    q, s, dq = quant_dynamic_oracle(np.array([0.0, -0.0], F32))  # amax = 0
    assert s == F32(448.0) and dq == F32(1.0) / F32(448.0) and list(q) == [0x00, 0x80]
    q, s, dq = quant_dynamic_oracle(np.array([0.5, -0.25, 2.0 ** -12], F32))  # amax < 1: 448 / amax = 896, the clamp of the scale bites
    assert s == F32(448.0) and list(e4m3_decode(q)) == [224.0, -112.0, 0.109375]
    # s = 1; f32 -> f16 drops the 2^-13, then 1.0625 is a tie that goes to the even 1.0 (0x38); rounding the f32 value directly gives 1.125 (0x39)
    q, s, dq = quant_dynamic_oracle(np.array([448.0, 1.0625 + 2.0 ** -13, -500.0], F32))
    assert s == F32(448.0) / F32(500.0) and dq == F32(1.0) / s
    q, s, dq = quant_dynamic_oracle(np.array([448.0, 1.0625 + 2.0 ** -13, -3.0], F32))
    assert s == 1.0 and dq == 1.0 and list(q) == [0x7E, 0x38, 0xC4]
    assert list(quant_static_oracle(np.array([1.0, -1000.0, 0.3], F32), 0.5)) == [0x40, 0xFE, list(encode([F32(0.3) / F32(0.5)]))[0]]


# ------------------------------------------------------------------------------------------------ UQFF serde type 3
def test_uqff_fp8_round_trip(tmp_path):
    g = torch.Generator().manual_seed(3)
    w = torch.randint(0, 0x7F, (8, 32), dtype=torch.uint8, generator=g)
    bias = torch.arange(8, dtype=torch.bfloat16)
    layer = fp8.FP8Linear.from_parts(w, bias, torch.tensor(0.25), torch.tensor(0.5), torch.tensor(4.0))
    path = str(tmp_path / "l.uqff")
    uqff.write(path, layer.serialize_uqff("m.q"))
    raw = open(path, "rb").read()
    header = json.loads(raw[8:8 + struct.unpack("<Q", raw[:8])[0]])
    mine = {k: v for k, v in header.items() if k.startswith("m.q.")}
    assert sorted(mine) == sorted("m.q." + s for s in ("weight", "weight.format", "weight.dequant_w_scale", "weight.dequant_x_scale", "weight.quant_scale",
                                                      "weight.dtype", "bias"))
    assert mine["m.q.weight"]["dtype"] == ("F8_E4M3" if hasattr(torch, "float8_e4m3fn") else "U8") and mine["m.q.weight"]["shape"] == [8, 32]
    assert all(mine[f"m.q.weight.{s}"] == dict(mine[f"m.q.weight.{s}"], dtype="F32", shape=[]) for s in ("dequant_w_scale", "dequant_x_scale", "quant_scale"))
    assert mine["m.q.weight.format"]["dtype"] == "U8" and mine["m.q.weight.dtype"]["dtype"] == "U32"
    r = uqff.UqffReader(path)
    assert r.serde_type("m.q") == uqff.SERDE_FP8 == 3 and r.isq_type("m.q") == "F8E4M3"
    full = fp8.fp8_linear_from_uqff(r, "m.q")
    assert torch.equal(full.weight.view(torch.uint8), w) and torch.equal(full.bias, bias) and r.load_fp8_layer("m.q").dtype_code == fp8.UQFF_DTYPE_F8E4M3
    assert [float(t) for t in (full.dequant_w_scale, full.dequant_x_scale, full.quant_scale)] == [0.25, 0.5, 4.0]
    half = r.load_fp8_layer("m.q", Shard(dim=0, rank=1, world_size=2))  # the N shard is the slice, of the weight and of the bias
    assert torch.equal(half.weight.view(torch.uint8), w[4:]) and torch.equal(half.bias, bias[4:]) and half.bias_mode == "narrow"
    cols = r.load_fp8_layer("m.q", Shard(dim=1, rank=0, world_size=2))  # a K shard: the caller adds the bias after the all-reduce
    assert torch.equal(cols.weight.view(torch.uint8), w[:, :16]) and cols.bias is None and cols.bias_mode == "skip"
    with pytest.raises(ValueError, match="is not an FP8 layer"):
        uqff.write(path, uqff.serialize_mxfp4_layer("m.q", np.zeros((2, 16), np.uint8), np.zeros((2, 1), np.uint8)))
        uqff.UqffReader(path).load_fp8_layer("m.q")


# ------------------------------------------------------------------------------------------------ loader
def test_pertensor_fp8_linear_b_branches():
    w, b = torch.zeros(8, 4, dtype=torch.uint8), torch.zeros(8, dtype=torch.float16)
    plain = fp8.pertensor_fp8_linear_b(4, 8, True, {"p.weight": torch.ones(8, 4), "p.bias": b}, "p")
    assert isinstance(plain, UnquantLinear) and plain.has_bias() and tuple(plain.dequantize_w().shape) == (8, 4)
    with pytest.raises(ValueError, match=r"cannot find tensor p\.weight, p\.weight_scale_inv"):
        fp8.pertensor_fp8_linear_b(4, 8, False, {}, "p")
    with pytest.raises(ValueError, match=r"cannot find tensor p\.weight$"):
        fp8.pertensor_fp8_linear_b(4, 8, False, {"p.weight_scale_inv": torch.tensor(1.0)}, "p")
    with pytest.raises(ValueError, match="shape mismatch for p.weight"):
        fp8.pertensor_fp8_linear_b(4, 9, False, {"p.weight": w, "p.weight_scale_inv": torch.tensor(1.0)}, "p")
    tensors = {"p.weight": w, "p.weight_scale_inv": torch.tensor(0.5), "p.activation_scale": torch.tensor(2.0), "p.bias": b}
    layer = fp8.pertensor_fp8_linear_b(4, 8, True, tensors, "p", act_quant="static")
    assert isinstance(layer, fp8.PerTensorFP8Linear) and layer.has_bias() and layer.dequant_dtype == torch.float16 and float(layer.activation_scale) == 2.0
    assert layer.name() == "pertensor-fp8-linear" and not layer.isq_serde_supported() and layer.act_quant == "static"
    nobias = fp8.pertensor_fp8_linear_b(4, 8, False, tensors, "p")
    assert not nobias.has_bias() and nobias.dequant_dtype == torch.bfloat16 and nobias.act_quant == "none"
    del tensors["p.activation_scale"]
    with pytest.raises(ValueError, match="needs an activation_scale"):
        fp8.pertensor_fp8_linear_b(4, 8, False, tensors, "p", act_quant="static")
    with pytest.raises(ValueError, match="Unknown act_quant"):
        fp8.pertensor_fp8_linear_b(4, 8, False, tensors, "p", act_quant="per-token")


# ------------------------------------------------------------------------------------------------ layer surface
def test_apply_isq_identities_and_errors():
    w = torch.zeros(8, 32, dtype=torch.uint8)
    one = torch.tensor(1.0)
    layer = fp8.FP8Linear.from_parts(w, None, one, one, one)
    assert layer.apply_isq(None) is layer and layer.apply_isq("F8E4M3") is layer and layer.apply_isq(None, [1.0] * 32) is layer
    with pytest.raises(ValueError, match="does not support imatrix"):
        layer.apply_isq("F8E4M3", [1.0] * 32)
    assert layer.name() == "fp8-linear" and layer.uqff_type() == "F8E4M3" and layer.isq_serde_supported() and not layer.has_bias()
    assert layer.dtype_and_device()[1] == torch.device("cpu") and layer.quantized_act_type() is None
    pt = fp8.PerTensorFP8Linear(w, one)
    with pytest.raises(ValueError, match="F8E4M3 does not support imatrix"):
        pt.apply_isq("F8E4M3", [1.0] * 32)
    with pytest.raises(ValueError, match="does not support add_delta_w"):
        pt.add_delta_w(torch.zeros(8, 32))
    for obj in (layer, pt):  # every other target dequantizes first, and that is a kernel
        with pytest.raises(ValueError, match="must live on the GPU"):
            obj.apply_isq("HQQ4")
        with pytest.raises(ValueError, match="must live on the GPU"):
            obj.forward(torch.zeros(1, 32, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="must live on the GPU"):
        fp8.FP8Linear.quantize(torch.zeros(8, 32))
    with pytest.raises(ValueError, match="Bias shape mismatch"):
        fp8.FP8Linear.from_parts(w, torch.zeros(7), one, one, one)
    with pytest.raises(ValueError, match="to be a scalar"):
        fp8.PerTensorFP8Linear(w, torch.ones(2))
    with pytest.raises(ValueError, match="u8 or float8_e4m3fn"):
        fp8.PerTensorFP8Linear(w.to(torch.int32), one)


# ------------------------------------------------------------------------------------------------ code objects
def test_fp8_pertensor_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    path = os.path.join(ROOT, "mistral.rs_amd", "lib", "libmistralrsquant.so")
    assert os.path.exists(path), "libmistralrsquant.so is not built"
    ks = [k for k in kernel_resources.resources(path) if "fp8_pertensor" in k["name"] or "fp8_pertensor" in k.get("demangled", "")]
    assert len(ks) >= 30, f"expected the per-tensor FP8 kernels in libmistralrsquant.so, found {len(ks)}"
    bad = [(k["demangled"], k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0), k.get("sgpr_spill_count", 0)) for k in ks
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0)]
    assert not bad, f"per-tensor FP8 kernels with scratch or spills: {bad}"
