"""CPU: the blockwise-FP8 host mirror -- the scale-shard rule and the module classification with the reference's own cases (blockwise_fp8/mod.rs:949-1108), the
config errors, the numpy E4M3 oracle the GPU test uses (pinned against torch's CPU float16 -> float8_e4m3fn conversion), argument errors, and the code
objects of the kernels (no scratch, no spills).  The GPU side is tests/test_zz_blockwise_fp8_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mistralrs_amd  # noqa: E402,F401
from mistralrs_amd import blockwise_fp8 as bf8  # noqa: E402
from mistralrs_amd.distributed import Shard  # noqa: E402


# ------------------------------------------------------------------------------------------------ the numpy oracle (shared with the GPU test)
def e4m3_decode(b: np.ndarray) -> np.ndarray:
    """OCP E4M3FN byte -> f64: bias 7, subnormals m * 2^-9, S.1111.111 = NaN, no infinities."""
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e.astype(np.float64) - 10))
    mag = np.where((e == 15) & (m == 7), np.nan, mag)
    return np.where(b & 0x80, -mag, mag)


def e4m3_encode_f16(h: np.ndarray) -> np.ndarray:
    """finite float16 -> E4M3FN byte, round to nearest even with saturation to +-448, in integer arithmetic on the f16 bit pattern.  E4M3's grid in units of
    2^-24 (the f16 subnormal quantum): an f16 value is the integer v = sig * 2^(max(e, 1) - 1) with sig = mant | (e ? 1024 : 0); E4M3 keeps 4 significant bits
    above 2^-6 = 2^18 units and a fixed step of 2^-9 = 2^15 units below."""
    bits = np.asarray(h, dtype=np.float16).view(np.uint16).astype(np.int64)
    sign, e, mant = (bits >> 8) & 0x80, (bits >> 10) & 31, bits & 1023
    v = (mant | np.where(e > 0, 1024, 0)) << (np.maximum(e, 1) - 1)      # |h| / 2^-24, exact (<= 2047 * 2^29 for |h| < 2^16)
    top = np.zeros_like(v)
    for i in range(1, 48):                                               # floor(log2 v), v > 0
        top += (v >> i) > 0
    shift = np.maximum(top - 3, 15)                                      # keep 4 bits, but never finer than 2^15 units
    q, rem = v >> shift, v & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))            # ties to even; the result is q * 2^shift units, q <= 16
    # shift == 15: q counts 2^-9 steps, which is the code itself (subnormals 0..7, exponent field 1 from 8 on); every further shift adds one to the exponent
    # field, and a carry to q == 16 lands on the next exponent by the same sum
    code = np.minimum(((shift - 15) << 3) + q, 0x7E)                     # satfinite: 448
    return (sign | code).astype(np.uint8)


def quant_oracle(w: np.ndarray, bsy: int, bsx: int):
    """The reference quantizer (blockwise_fp8.cu:68-139) on f32 values: scale = max(absmax / 448, 1e-12) in f32, q = e4m3(f16(clamp(v / scale)))."""
    w = np.asarray(w, dtype=np.float32)
    h, wd = w.shape
    gy, gx = -(-h // bsy), -(-wd // bsx)
    scale, q = np.zeros((gy, gx), np.float32), np.zeros((h, wd), np.uint8)
    for i in range(gy):
        for j in range(gx):
            blk = w[i * bsy:(i + 1) * bsy, j * bsx:(j + 1) * bsx]
            s = np.maximum(np.float32(np.max(np.abs(blk))) / np.float32(448.0), np.float32(1e-12)).astype(np.float32)
            scale[i, j] = s
            v = np.clip((blk / s).astype(np.float32), np.float32(-448.0), np.float32(448.0))
            q[i * bsy:(i + 1) * bsy, j * bsx:(j + 1) * bsx] = e4m3_encode_f16(v.astype(np.float16))
    return q, scale


@pytest.mark.skipif(not hasattr(torch, "float8_e4m3fn"), reason="this torch has no float8_e4m3fn")
def test_numpy_e4m3_oracle_matches_torch_over_all_f16():
    allbits = np.arange(65536, dtype=np.uint16).view(np.float16)
    with np.errstate(invalid="ignore"):
        h = allbits[np.isfinite(allbits) & (np.abs(allbits.astype(np.float32)) <= 448.0)]
    assert h.size == 2 * (0x5F00 + 1) and (h == np.float16(448.0)).any() and (h.view(np.uint16) == 0x8000).any()
    want = torch.from_numpy(h.copy()).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = e4m3_encode_f16(h)
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{len(bad)} of {h.size} differ; first: f16 {h[bad[0]]!r} -> oracle {got[bad[0]]:#x}, torch {want[bad[0]]:#x}"
    # and the decoder is the inverse on every non-NaN byte, torch's decode included
    codes = np.arange(256, dtype=np.uint8)
    dec = e4m3_decode(codes)
    tdec = torch.from_numpy(codes).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(dec), np.isnan(tdec)) and np.isnan(dec).sum() == 2
    ok = ~np.isnan(dec)
    assert np.array_equal(dec[ok], tdec[ok]) and np.array_equal(np.signbit(dec[ok]), np.signbit(tdec[ok]))
    assert np.array_equal(e4m3_encode_f16(dec[ok].astype(np.float16)), codes[ok])


def test_quant_oracle_double_rounding_pin():
    w = np.zeros((1, 4), np.float32)
    w[0] = [448.0, 1.0625 + 2.0 ** -13, -448.0, -0.0]
    q, s = quant_oracle(w, 128, 128)
    assert s[0, 0] == 1.0 and list(q[0]) == [0x7E, 0x38, 0xFE, 0x80]  # f32 -> f16 drops the 2^-13, then 1.0625 is a tie that goes to the even 1.0
    q, s = quant_oracle(np.zeros((2, 2), np.float32), 128, 128)
    assert s[0, 0] == np.float32(1e-12) and not q.any()


# ------------------------------------------------------------------------------------------------ scale_shard_from_weight_shard (mod.rs:949-1044)
def test_scale_shard_follows_simple_weight_partition():
    assert bf8.scale_shard_from_weight_shard((12288, 5120), (128, 128), Shard(dim=0, rank=3, world_size=8)) == Shard(dim=0, offset=36, length=12)
    assert bf8.scale_shard_from_weight_shard((5120, 6144), (128, 128), Shard(dim=1, rank=7, world_size=8)) == Shard(dim=1, offset=42, length=6)


def test_scale_shard_maps_replicated_kv_offset_to_scale_rows():
    assert bf8.scale_shard_from_weight_shard((1024, 5120), (128, 128), Shard(dim=0, offset=512, length=256)) == Shard(dim=0, offset=4, length=2)


def test_derived_scale_offset_selects_matching_scale_blocks():
    scales = torch.arange(1.0, 9.0).reshape(4, 2)
    sh = bf8.scale_shard_from_weight_shard((8, 4), (2, 2), Shard(dim=0, offset=4, length=2))
    assert bf8._apply_shard(scales, sh).tolist() == [[5.0, 6.0]]


def test_scale_shard_rejects_unaligned_weight_partition():
    with pytest.raises(ValueError, match="not aligned"):
        bf8.scale_shard_from_weight_shard((1024, 5120), (128, 128), Shard(dim=0, offset=64, length=256))
    with pytest.raises(ValueError, match="not aligned"):
        bf8.scale_shard_from_weight_shard((1024, 5120), (128, 128), Shard(dim=0, offset=128, length=64))
    with pytest.raises(ValueError, match="exceeds dimension size"):
        bf8.scale_shard_from_weight_shard((1024, 5120), (128, 128), Shard(dim=0, offset=896, length=256))
    with pytest.raises(ValueError, match="not divisible by world size"):
        bf8.scale_shard_from_weight_shard((1000, 5120), (128, 128), Shard(dim=0, rank=0, world_size=3))
    with pytest.raises(ValueError, match="Invalid FP8 weight shard rank"):
        bf8.scale_shard_from_weight_shard((1024, 5120), (128, 128), Shard(dim=0, rank=2, world_size=2))


def test_last_scale_shard_may_end_off_block_at_the_dimension_end():
    # 1000 rows = 7 whole blocks + 104: the shard 896..1000 ends at the dimension's end and owns the partial block
    assert bf8.scale_shard_from_weight_shard((1000, 512), (128, 128), Shard(dim=0, offset=896, length=104)) == Shard(dim=0, offset=7, length=1)
    assert bf8.scale_shard_from_weight_shard((1000, 512), (128, 128), Shard(dim=0, offset=0, length=1000)) == Shard(dim=0, offset=0, length=8)


# ------------------------------------------------------------------------------------------------ module kind / linear_b (mod.rs:1045-1108)
def fp8_config(exclusions=(), **over):
    cfg = {"quant_method": "fp8", "weight_block_size": [128, 128], "activation_scheme": "dynamic", "fmt": "e4m3", "modules_to_not_convert": list(exclusions)}
    cfg.update(over)
    return cfg


def test_excluded_fp8_linear_preserves_weight_shard():
    tensors = {"foo.weight": torch.arange(32.0).reshape(8, 4)}
    layer = bf8.blockwise_fp8_linear_b(4, 8, fp8_config(["foo"]), False, Shard(dim=0, rank=1, world_size=2), tensors, "foo")
    assert isinstance(layer, bf8.UnquantLinear) and tuple(layer.dequantize_w().shape) == (4, 4)
    assert torch.equal(layer.dequantize_w(), tensors["foo.weight"][4:])


def test_official_language_model_alias_is_excluded():
    tensors = {"model.language_model.embed_tokens.weight": torch.zeros(8, 4)}
    layer = bf8.blockwise_fp8_linear_b(4, 8, fp8_config(["model.embed_tokens"]), False, None, tensors, "model.language_model.embed_tokens")
    assert isinstance(layer, bf8.UnquantLinear) and tuple(layer.dequantize_w().shape) == (8, 4)
    assert bf8.blockwise_fp8_module_kind(fp8_config(["language_model.model.embed_tokens"]), tensors, "model.language_model.embed_tokens") == "unquantized"
    assert bf8._canonical_language_model_module_path("other.model.embed_tokens") != bf8._canonical_language_model_module_path("model.embed_tokens")


def test_declared_exclusions_make_unlisted_missing_scale_an_error():
    tensors = {"foo.weight": torch.zeros(8, 4)}
    with pytest.raises(ValueError, match="not listed"):
        bf8.blockwise_fp8_linear_b(4, 8, fp8_config(["bar"]), False, None, tensors, "foo")
    # nothing declared excluded: a scale-less module is simply unquantized
    assert bf8.blockwise_fp8_module_kind(fp8_config(), tensors, "foo") == "unquantized"
    assert bf8.blockwise_fp8_module_kind(fp8_config(), tensors, "nope") == "missing"
    with pytest.raises(ValueError, match="cannot find tensor"):
        bf8.blockwise_fp8_linear_b(4, 8, fp8_config(), False, None, tensors, "nope")


def test_excluded_module_with_a_scale_is_an_error():
    tensors = {"foo.weight": torch.zeros(8, 4, dtype=torch.uint8), "foo.weight_scale_inv": torch.ones(1, 1)}
    with pytest.raises(ValueError, match="unexpectedly has `weight_scale_inv`"):
        bf8.blockwise_fp8_module_kind(fp8_config(["foo"]), tensors, "foo")
    assert bf8.blockwise_fp8_module_kind(fp8_config(["bar"]), tensors, "foo") == "quantized"


def test_linear_b_config_errors_and_cpu_load():
    tensors = {"foo.weight": torch.zeros(8, 4, dtype=torch.uint8), "foo.weight_scale_inv": torch.ones(1, 1), "foo.bias": torch.zeros(8)}
    with pytest.raises(ValueError, match="requires weight_block_size to be set"):
        bf8.blockwise_fp8_linear_b(4, 8, fp8_config(weight_block_size=None), False, None, tensors, "foo")
    with pytest.raises(ValueError, match="to have length 2"):
        bf8.blockwise_fp8_linear_b(4, 8, fp8_config(weight_block_size=[128]), False, None, tensors, "foo")
    with pytest.raises(ValueError, match="nonzero weight_block_size"):
        bf8.blockwise_fp8_linear_b(4, 8, fp8_config(weight_block_size=[128, 0]), False, None, tensors, "foo")
    with pytest.raises(ValueError, match="Unsupported blockwise FP8 format"):
        bf8.blockwise_fp8_linear_b(4, 8, fp8_config(fmt="e5m2"), False, None, tensors, "foo")
    with pytest.raises(ValueError, match="Unexpected quantization config"):
        bf8.blockwise_fp8_linear_b(4, 8, {"quant_method": "gptq"}, False, None, tensors, "foo")
    layer = bf8.blockwise_fp8_linear_b(4, 8, fp8_config(fmt=None), True, None, tensors, "foo")  # the pure load works on the CPU
    assert isinstance(layer, bf8.BlockwiseFP8Linear) and layer.has_bias() and layer.weight_block_size == (128, 128) and layer.activation_scheme == "dynamic"
    assert layer.name() == "blockwise-fp8-linear" and not layer.isq_serde_supported() and layer.quantized_act_type() is None
    assert layer.dtype_and_device()[1] == torch.device("cpu")


def test_layer_argument_errors():
    w, s = torch.zeros(6, 200, dtype=torch.uint8), torch.ones(1, 2)
    with pytest.raises(ValueError, match="u8 or float8_e4m3fn"):
        bf8.BlockwiseFP8Linear(w.to(torch.int32), s)
    with pytest.raises(ValueError, match="Scale shape mismatch"):
        bf8.BlockwiseFP8Linear(w, torch.ones(1, 3))
    with pytest.raises(ValueError, match="f32 tensor"):
        bf8.BlockwiseFP8Linear(w, s.to(torch.float16))
    with pytest.raises(ValueError, match="to have length 2"):
        bf8.BlockwiseFP8Linear(w, s, weight_block_size=(128,))
    with pytest.raises(ValueError, match="nonzero weight_block_size"):
        bf8.BlockwiseFP8Linear(w, s, weight_block_size=(0, 128))
    with pytest.raises(ValueError, match="Bias shape mismatch"):
        bf8.BlockwiseFP8Linear(w, s, bias=torch.zeros(5))
    layer = bf8.BlockwiseFP8Linear(w, s)
    with pytest.raises(ValueError, match="must live on the GPU"):
        layer.forward(torch.zeros(1, 200, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="must live on the GPU"):
        layer.dequantize_w()
    with pytest.raises(ValueError, match="must live on the GPU"):
        bf8.BlockwiseFP8Linear.quantize(torch.zeros(4, 4))
    with pytest.raises(ValueError, match=r"expected \[num_experts, N, K\]"):
        layer.gather_forward(torch.zeros(1, 200, dtype=torch.bfloat16), torch.zeros(1, 2, dtype=torch.int32))
    experts = bf8.blockwise_fp8_moe(torch.zeros(2, 6, 200, dtype=torch.uint8), torch.ones(2, 1, 2), [128, 128])
    assert not experts.has_bias()
    with pytest.raises(ValueError, match="stacked experts go through gather_forward"):
        experts.forward(torch.zeros(1, 200, dtype=torch.bfloat16))
    if hasattr(torch, "float8_e4m3fn"):
        assert bf8.BlockwiseFP8Linear(w.view(torch.float8_e4m3fn), s).weight.dtype == torch.uint8


# ------------------------------------------------------------------------------------------------ code objects
def test_blockwise_fp8_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    path = os.path.join(ROOT, "mistral.rs_amd", "lib", "libmistralrsquant.so")
    assert os.path.exists(path), "libmistralrsquant.so is not built"
    mine = lambda k: any(t in k["name"] or t in k.get("demangled", "") for t in ("fp8_blockwise", "blockwise_fp8"))
    ks = [k for k in kernel_resources.resources(path) if mine(k)]
    assert len(ks) >= 10, f"expected the blockwise FP8 kernels in libmistralrsquant.so, found {len(ks)}"
    bad = [(k["demangled"], k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0), k.get("sgpr_spill_count", 0)) for k in ks
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0)]
    assert not bad, f"blockwise FP8 kernels with scratch or spills: {bad}"
    tiles = [k for k in ks if "tile" in k.get("demangled", k["name"])]
    assert tiles and all(k.get("vgpr_count", 0) <= 256 for k in tiles), [(k["demangled"], k.get("vgpr_count")) for k in tiles]
