"""CPU: the MXFP4 host mirror -- quantizer rule, UQFF round trips and shard rule, and the code objects of the MXFP4 kernels (no scratch, no spills).
The GPU side is tests/test_zz_mxfp4_gpu.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mistralrs_amd  # noqa: E402,F401
from mistralrs_amd import mxfp4, uqff  # noqa: E402
from mistralrs_amd.distributed import Shard  # noqa: E402

FP4 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def ref_nibble(val: float) -> int:  # mod.rs:427-457
    a = abs(val)
    nib = 0 if a < 0.25 else 1 if a < 0.75 else 2 if a < 1.25 else 3 if a < 1.75 else 4 if a < 2.5 else 5 if a < 3.5 else 6 if a < 5.0 else 7
    return nib | 8 if val < 0.0 else nib


def ref_quantize(w: np.ndarray):
    """A plain loop restating mod.rs:368-399 (f32 values, f32 products by powers of two are exact)."""
    n, k = w.shape
    packed, scales = np.zeros((n, k // 2), np.uint8), np.zeros((n, k // 32), np.uint8)
    for row in range(n):
        for blk in range(k // 32):
            block = w[row, blk * 32:(blk + 1) * 32]
            max_abs = float(np.max(np.abs(block)))
            scale = 127 if max_abs == 0.0 else min(max(math.floor(math.log2(float(np.float32(max_abs) / np.float32(6.0)))) + 127, 0), 254)
            scales[row, blk] = scale
            inv = 2.0 ** (127 - scale)
            for e, v in enumerate(block):
                nib = ref_nibble(float(v) * inv)
                kk = blk * 32 + e
                packed[row, kk // 2] |= nib if kk % 2 == 0 else nib << 4
    return packed, scales


def reference_vector():
    return ((np.arange(7 * 64) % 29).astype(np.float32) - np.float32(14.0)) / np.float32(3.0)  # mod.rs:939-945


def test_quantizer_matches_the_reference_rule():
    w = reference_vector().reshape(7, 64)
    want_b, want_s = ref_quantize(w)
    layer = mxfp4.MXFP4Layer.quantize(torch.from_numpy(w))
    assert layer.blocks.dtype == torch.uint8 and tuple(layer.blocks.shape) == (7, 32) and tuple(layer.scales.shape) == (7, 2)
    assert np.array_equal(layer.scales.numpy(), want_s)
    assert np.array_equal(layer.blocks.numpy(), want_b)
    assert layer.uqff_type() == "MXFP4" and not layer.has_bias() and layer.dtype_and_device()[0] == torch.bfloat16


def test_quantizer_zero_block_thresholds_and_nibble_order():
    w = np.zeros((2, 64), np.float32)
    # row 0, block 1: max 6 -> scale 127 (factor 1); one value on each decision boundary, and the negative ones
    bounds = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    w[0, 32] = 6.0
    w[0, 33:40] = bounds
    w[0, 40:47] = [-b for b in bounds]
    w[0, 47] = 0.2499
    # row 1, block 0: nibble order -- k = 0 -> 1.0 (nibble 2), k = 1 -> -6.0 (nibble 15)
    w[1, 0], w[1, 1] = 1.0, -6.0
    blocks, scales = mxfp4.quantize_tensors(torch.from_numpy(w))
    blocks, scales = blocks.numpy(), scales.numpy()
    assert scales[0, 0] == 127  # all-zero block
    assert scales[0, 1] == 127 and scales[1, 0] == 127 and scales[1, 1] == 127
    nib = np.stack([blocks & 15, blocks >> 4], -1).reshape(2, 64)
    assert list(nib[0, 32:48]) == [7, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 0]  # every boundary value lands on the upper side
    assert blocks[1, 0] == (15 << 4 | 2)  # low nibble = even k
    want_b, want_s = ref_quantize(w)
    assert np.array_equal(blocks, want_b) and np.array_equal(scales, want_s)
    # scale range: clamp at 0 and 254, powers of two exactly
    big = np.zeros((1, 96), np.float32)
    big[0, 0], big[0, 32], big[0, 64] = 3e38, 1e-44, 12.0
    _, s = mxfp4.quantize_tensors(torch.from_numpy(big))
    assert list(s.numpy()[0]) == [min(math.floor(math.log2(3e38 / 6)) + 127, 254), 0, 128]
    with pytest.raises(ValueError, match="divisible by block size"):
        mxfp4.quantize_tensors(torch.zeros(2, 48))


def _layer(rank, with_bias, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape = (3, 6, 128) if rank == 3 else (6, 128)
    blocks = torch.randint(0, 256, (*shape[:-1], shape[-1] // 2), dtype=torch.uint8, generator=g)
    scales = torch.randint(107, 138, (*shape[:-1], shape[-1] // 32), dtype=torch.uint8, generator=g)
    bias = torch.randn(shape[:-1], generator=g).to(torch.bfloat16) if with_bias else None
    return blocks, scales, bias


@pytest.mark.parametrize("rank", [2, 3])
@pytest.mark.parametrize("with_bias", [False, True])
def test_uqff_round_trip(tmp_path, rank, with_bias):
    blocks, scales, bias = _layer(rank, with_bias)
    layer = mxfp4.MXFP4Layer.from_parts(blocks, scales, bias)
    entries = layer.serialize_uqff("model.layers.0.mlp")
    assert list(entries)[:3] == ["model.layers.0.mlp.weight.format", "model.layers.0.mlp.weight", "model.layers.0.mlp.weight.scales"]
    assert int(entries["model.layers.0.mlp.weight.format"]) == uqff.SERDE_MXFP4 == 6
    assert ("model.layers.0.mlp.bias" in entries) == with_bias
    path = str(tmp_path / "m.uqff")
    uqff.write(path, entries)
    r = uqff.UqffReader(path)
    assert r.isq_type("model.layers.0.mlp") == "MXFP4"
    back = mxfp4.MXFP4Layer.from_uqff(r, "model.layers.0.mlp", "cpu")
    assert torch.equal(back.blocks, blocks) and torch.equal(back.scales, scales)
    assert (back.bias is None) == (not with_bias)
    if with_bias:
        assert back.bias.dtype == torch.bfloat16 and torch.equal(back.bias, bias)


def test_uqff_shards(tmp_path):
    blocks, scales, bias = _layer(2, True)   # N = 6, K = 128
    path = str(tmp_path / "s.uqff")
    uqff.write(path, uqff.serialize_mxfp4_layer("l", blocks, scales, bias))
    r = uqff.UqffReader(path)
    # last dim, world 2: K 64..128 -> bytes 32..64, scale bytes 2..4; the bias of an input-dim shard is the caller's to add
    d = r.load_mxfp4_layer("l", Shard(dim=1, rank=1, world_size=2))
    assert torch.equal(d.blocks, blocks[:, 32:64]) and torch.equal(d.scales, scales[:, 2:4]) and d.bias is None and d.bias_mode == "skip"
    d = r.load_mxfp4_layer("l", Shard(dim=1, rank=0, world_size=2))
    assert torch.equal(d.blocks, blocks[:, :32]) and torch.equal(d.scales, scales[:, :2])
    with pytest.raises(ValueError, match="Sharding the MXFP4 packed dim requires alignment of 32: start 16, len 32."):
        r.load_mxfp4_layer("l", Shard(dim=1, offset=16, length=32))
    with pytest.raises(ValueError, match="requires alignment of 32"):
        r.load_mxfp4_layer("l", Shard(dim=1, offset=32, length=48))
    # dim 0: both tensors and the bias
    d = r.load_mxfp4_layer("l", Shard(dim=0, rank=1, world_size=3))
    assert torch.equal(d.blocks, blocks[2:4]) and torch.equal(d.scales, scales[2:4]) and torch.equal(d.bias, bias[2:4]) and d.bias_mode == "narrow"
    # stacked experts: dim 1 is the output dim of every expert
    b3, s3, bias3 = _layer(3, True, seed=1)
    path3 = str(tmp_path / "s3.uqff")
    uqff.write(path3, uqff.serialize_mxfp4_layer("e", b3, s3, bias3))
    d = uqff.UqffReader(path3).load_mxfp4_layer("e", Shard(dim=1, rank=1, world_size=2))
    assert torch.equal(d.blocks, b3[:, 3:6]) and torch.equal(d.scales, s3[:, 3:6]) and torch.equal(d.bias, bias3[:, 3:6])
    d = uqff.UqffReader(path3).load_mxfp4_layer("e", Shard(dim=2, rank=1, world_size=2))
    assert torch.equal(d.blocks, b3[:, :, 32:]) and torch.equal(d.scales, s3[:, :, 2:]) and d.bias is None
    with pytest.raises(ValueError, match="not an MXFP4 layer|Missing"):
        uqff.UqffReader(path3).load_mxfp4_layer("nope")


def test_layer_argument_errors():
    blocks, scales, _ = _layer(2, False)
    with pytest.raises(ValueError, match="Scale shape mismatch"):
        mxfp4.MXFP4Layer.from_parts(blocks, scales[:, :3])
    with pytest.raises(ValueError, match="u8"):
        mxfp4.MXFP4Layer.from_parts(blocks.to(torch.int32), scales)
    with pytest.raises(ValueError, match="must live on the GPU"):
        mxfp4.MXFP4Layer.from_parts(blocks, scales).forward(torch.zeros(1, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r"num_experts, out_dim, num_blocks, 16"):
        mxfp4.packed_gptoss_blocks(torch.zeros(2, 8, 48, dtype=torch.uint8))
    assert tuple(mxfp4.packed_gptoss_blocks(torch.zeros(2, 8, 3, 16, dtype=torch.uint8)).shape) == (2, 8, 48)


@pytest.mark.parametrize("lib", ["libmistralrsquant.so", "libmrs_hip_ext.so"])
def test_mxfp4_kernels_use_no_scratch(lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    path = os.path.join(ROOT, "mistral.rs_amd", "lib", lib)
    assert os.path.exists(path), f"{lib} is not built"
    ks = [k for k in kernel_resources.resources(path) if "mxfp4" in k["name"] or "mxfp4" in k.get("demangled", "")]
    assert ks, f"no mxfp4 kernel in {lib}"
    bad = [(k["demangled"], k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0)) for k in ks
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0)]
    assert not bad, f"mxfp4 kernels with scratch or VGPR spills: {bad}"
