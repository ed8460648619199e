"""CPU: AFQ -- a numpy oracle written from the format definition (pack, unpack, quantize, dequantize; the GPU file imports it), the reference's round-trip
and embedding cases, hand-checked pins, UQFF round trips and the shard rule, the host mirror's argument checks, and the code objects of the AFQ kernels (no
scratch, no spills, VGPR / LDS inside the limits).  The GPU side is tests/test_zz_afq_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import mistralrs_amd  # noqa: E402,F401
from mistralrs_amd import afq, uqff  # noqa: E402
from mistralrs_amd.distributed import Shard  # noqa: E402

BITS = [2, 3, 4, 6, 8]
GROUPS = [32, 64, 128]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


# ------------------------------------------------------------------------------------------------ oracle
def pack(codes: np.ndarray, bits: int) -> np.ndarray:
    """codes [.., K] -> u32 [.., K * bits / 32]: element j in bits [j * bits, (j + 1) * bits) of the row's little-endian bit stream"""
    codes = np.asarray(codes, dtype=np.uint32)
    k = codes.shape[-1]
    assert (k * bits) % 32 == 0 and codes.max(initial=0) < (1 << bits)
    stream = ((codes[..., None] >> np.arange(bits, dtype=np.uint32)) & 1).astype(np.uint8).reshape(*codes.shape[:-1], k * bits)
    words = stream.reshape(*codes.shape[:-1], k * bits // 32, 32).astype(np.uint64)
    return (words << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack(w_q: np.ndarray, bits: int) -> np.ndarray:
    w_q = np.asarray(w_q, dtype=np.uint32)
    stream = ((w_q[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(*w_q.shape[:-1], -1)
    k = stream.shape[-1] // bits
    return (stream.reshape(*w_q.shape[:-1], k, bits).astype(np.uint32) << np.arange(bits, dtype=np.uint32)).sum(-1).astype(np.uint32)


def quantize(w: torch.Tensor, bits: int, group: int):
    """The reference's CPU quantizer (afq/ops.rs:1534-1622) on a torch tensor of dtype T: f32 arithmetic throughout, unrounded f32 scale and bias for the codes,
    round half away from zero; scales and biases come back as T."""
    wf = w.detach().to(torch.float32).numpy()
    g = wf.reshape(*wf.shape[:-1], wf.shape[-1] // group, group)
    lo, hi = g.min(-1), g.max(-1)
    levels = np.float32((1 << bits) - 1)
    rng = (hi - lo).astype(np.float32)
    scale = np.where(np.abs(rng) < np.float32(1e-12), np.float32(1.0), (rng / levels).astype(np.float32)).astype(np.float32)
    t = ((g - lo[..., None]).astype(np.float32) / scale[..., None]).astype(np.float32)
    # roundf: t + 0.5 is exact in f64 (in f32 the sum itself could round, e.g. at 0.5 - 1 ulp)
    q = np.clip(np.where(t >= 0, np.floor(t.astype(np.float64) + 0.5), np.ceil(t.astype(np.float64) - 0.5)), 0, float(levels))
    codes = q.astype(np.uint32).reshape(wf.shape)
    return pack(codes, bits), torch.from_numpy(scale).to(w.dtype), torch.from_numpy(lo.astype(np.float32)).to(w.dtype)


def dequantize_f64(w_q: np.ndarray, scales: torch.Tensor, biases: torch.Tensor, bits: int, group: int) -> np.ndarray:
    q = unpack(w_q, bits).astype(np.float64)
    s, b = scales.double().numpy(), biases.double().numpy()
    return q * np.repeat(s, group, -1) + np.repeat(b, group, -1)


def dequantize(w_q, scales, biases, bits, group) -> torch.Tensor:
    """T(fmaf(q, s, b)) computed as f64 q * s + b -> f32 -> T (the f64 value is exact: 8 + 24 bits; callers with f32 parts assert no f32 tie)"""
    return torch.from_numpy(dequantize_f64(w_q, scales, biases, bits, group).astype(np.float32)).to(scales.dtype)


def no_f32_ties(v64: np.ndarray) -> bool:
    """no f64 value sits exactly halfway between two f32 neighbours"""
    f = v64.astype(np.float32)
    nb = np.nextafter(f, np.where(v64 > f, np.inf, -np.inf).astype(np.float32))
    mid = (f.astype(np.float64) + nb.astype(np.float64)) / 2
    return not np.any((v64 != f) & (v64 == mid))


# ------------------------------------------------------------------------------------------------ oracle checks
def test_pack_unpack_round_trip_and_straddles():
    rng = np.random.default_rng(0)
    for bits in BITS:
        codes = rng.integers(0, 1 << bits, (3, 96), dtype=np.uint32)
        w_q = pack(codes, bits)
        assert w_q.shape == (3, 96 * bits // 32) and np.array_equal(unpack(w_q, bits), codes)
    # 3 bits: element 10 occupies bits 30..32 -> the low 2 bits end word 0, the top bit starts word 1
    c = np.zeros((1, 32), np.uint32)
    c[0, 10] = 0b101
    assert list(pack(c, 3)[0]) == [0b01 << 30, 0b1, 0]
    # 6 bits: element 5 occupies bits 30..35
    c = np.zeros((1, 32), np.uint32)
    c[0, 5] = 0b110110
    assert list(pack(c, 6)[0]) == [(0b10 << 30), 0b1101, 0, 0, 0, 0]
    # the reference's byte-wise extract_3bit / extract_6bit read the same stream: bytes little-endian
    c = rng.integers(0, 8, (1, 32), dtype=np.uint32)
    by = pack(c, 3).view(np.uint8)[0]
    bitstream = np.unpackbits(by, bitorder="little")
    assert np.array_equal((bitstream.reshape(32, 3) << np.arange(3)).sum(-1), c[0])


@pytest.mark.parametrize("bits,limit", [(8, 0.005), (6, 0.02), (4, 0.09), (3, 0.17), (2, 0.40)])
def test_reference_round_trip_rmse(bits, limit):
    i = np.arange(32 * 64, dtype=np.float32)
    xs = (np.sin(i * np.float32(0.013)) + np.cos(i * np.float32(0.017)) * np.float32(0.5)).astype(np.float32).reshape(32, 64)
    w_q, s, b = quantize(torch.from_numpy(xs), bits, 32)
    ys = dequantize(w_q, s, b, bits, 32).numpy()
    rmse = float(np.mean(np.sqrt(np.mean((xs - ys) ** 2, -1))))
    assert rmse < limit, rmse


@pytest.mark.parametrize("bits", BITS)
def test_reference_embedding_case(bits):
    i = np.arange(16 * 64, dtype=np.float32)
    xs = (np.sin(i * np.float32(0.011)) - np.cos(i * np.float32(0.019)) * np.float32(0.25)).astype(np.float32).reshape(16, 64)
    w_q, s, b = quantize(torch.from_numpy(xs), bits, 32)
    ids = np.array([[3, 1], [3, 15]])
    got = dequantize(w_q[ids.reshape(-1)], s[ids.reshape(-1)], b[ids.reshape(-1)], bits, 32).reshape(2, 2, 64)
    want = dequantize(w_q, s, b, bits, 32)[ids.reshape(-1)].reshape(2, 2, 64)
    assert torch.equal(got, want) and float((got - torch.from_numpy(xs)[ids.reshape(-1)].reshape(2, 2, 64)).abs().max()) < 1.0


def test_quantizer_pins():
    # a constant group: scale 1.0, codes 0, bias the constant
    w = torch.full((1, 32), 0.75)
    w_q, s, b = quantize(w, 4, 32)
    assert not w_q.any() and float(s[0, 0]) == 1.0 and float(b[0, 0]) == 0.75
    # half-away tie: range 0..15 at 4 bits -> scale 1; 2.5 -> 3, 0.5 -> 1 (half to even would give 2 and 0)
    v = np.zeros((1, 32), np.float32)
    v[0, 1], v[0, 2], v[0, 3] = 15.0, 2.5, 0.5
    w_q, s, b = quantize(torch.from_numpy(v), 4, 32)
    assert float(s[0, 0]) == 1.0 and list(unpack(w_q, 4)[0, :4]) == [0, 15, 3, 1]
    # scale / bias rounding: the codes use the f32 values, the stored ones are RNE to T
    v = np.zeros((1, 32), np.float32)
    v[0, 0], v[0, 1] = 1.0 + 2.0 ** -9, 2.0   # 1 + 2^-9 is an f16 value; bf16 stores 1.0
    for dt in (torch.float16, torch.bfloat16):
        w = torch.from_numpy(v).to(dt)        # T inputs: the quantizer widens what is stored
        w_q, s, b = quantize(w, 8, 32)
        wf = w.float().numpy()
        lo, hi = wf.min(), wf.max()
        assert float(b[0, 0]) == float(torch.tensor(lo).to(dt)) and float(s[0, 0]) == float(torch.tensor(np.float32(hi - lo) / np.float32(255)).to(dt))
        assert float(s[0, 0]) != float(np.float32(hi - lo) / np.float32(255))  # the stored scale did round
        assert unpack(w_q, 8)[0, 1] == 255 or lo == wf[0, 1]
    # range underflow in f16: tiny range, f32 scale ~1e-9 stores as 0 in f16 while the codes still spread over the levels
    v = np.full((1, 32), 1e-7, np.float32)
    v[0, 1] = 3e-7
    w = torch.from_numpy(v).to(torch.float16)
    w_q, s, b = quantize(w, 2, 32)
    assert unpack(w_q, 2)[0, 1] == 3 and float(s[0, 0]) < 1e-7


# ------------------------------------------------------------------------------------------------ UQFF
def _layer(rank, with_bias, bits=4, group=64, dt=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape = (3, 6, 128) if rank == 3 else (6, 128)
    w_q = torch.randint(0, 2 ** 31 - 1, (*shape[:-1], shape[-1] * bits // 32), dtype=torch.int32, generator=g).view(torch.uint32)
    scales = torch.randn((*shape[:-1], shape[-1] // group), generator=g).to(dt)
    biases = torch.randn((*shape[:-1], shape[-1] // group), generator=g).to(dt)
    bias = torch.randn(shape[:-1], generator=g).to(dt) if with_bias else None
    return w_q, scales, biases, bias


def _eq(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.uint32 else a, b.view(torch.int32) if b.dtype == torch.uint32 else b)


@pytest.mark.parametrize("rank", [2, 3])
@pytest.mark.parametrize("with_bias", [False, True])
def test_uqff_round_trip_and_header(tmp_path, rank, with_bias):
    w_q, scales, biases, bias = _layer(rank, with_bias, bits=6, group=32)
    layer = afq.AfqLayer.from_parts(w_q, scales, biases, bias, 6, 32)
    entries = layer.serialize_uqff("m.l")
    want = ["m.l.weight.format", "m.l.weight.bits", "m.l.weight.group_size", "m.l.weight", "m.l.weight.scales", "m.l.weight.biases"] + (["m.l.bias"] if with_bias else [])
    assert list(entries) == want
    assert int(entries["m.l.weight.format"]) == uqff.SERDE_AFQ == 4 and int(entries["m.l.weight.bits"]) == 6 and int(entries["m.l.weight.group_size"]) == 32
    assert all(entries[k].dtype == np.uint8 and entries[k].shape == () for k in want[:3])
    path = str(tmp_path / "m.uqff")
    uqff.write(path, entries)
    r = uqff.UqffReader(path)
    assert r.isq_type("m.l") == "AFQ6" and r.serde_type("m.l") == 4
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:  # the raw file: names and stored dtypes
        assert set(want) <= set(f.keys()) and f.get_tensor("m.l.weight").dtype == torch.uint32 and f.get_tensor("m.l.weight.scales").dtype == torch.bfloat16
    back = afq.AfqLayer.from_uqff(r, "m.l", "cpu")
    assert _eq(back.w_q, w_q) and _eq(back.scales, scales) and _eq(back.biases, biases) and back.bits == 6 and back.group_size == 32
    assert (back.bias is None) == (not with_bias) and back.uqff_type() == "AFQ6"
    if with_bias:
        assert _eq(back.bias, bias)


def test_uqff_three_and_six_bit_shards(tmp_path):
    """The reference's test (afq/mod.rs:622-684): 2 x 128 at group 32, whole and as rank 1 of a world-2 last-dim shard."""
    n, k, group = 2, 128, 32
    entries = {}
    for prefix, bits in (("afq3", 3), ("afq6", 6)):
        entries.update(uqff.serialize_afq_layer(prefix, torch.zeros(n, k * bits // 32, dtype=torch.uint32), torch.zeros(n, k // group, dtype=torch.bfloat16),
                                                torch.zeros(n, k // group, dtype=torch.bfloat16), bits, group))
    path = str(tmp_path / "afq-3-6.uqff")
    uqff.write(path, entries)
    r = uqff.UqffReader(path)
    for prefix, bits in (("afq3", 3), ("afq6", 6)):
        full = r.load_afq_layer(prefix)
        assert tuple(full.w_q.shape) == (n, k * bits // 32) and tuple(full.scales.shape) == (n, k // group)
        assert dequantize(full.w_q.view(torch.int32).numpy().view(np.uint32), full.scales, full.biases, bits, group).shape == (n, k)
        part = r.load_afq_layer(prefix, Shard(dim=1, rank=1, world_size=2))
        assert tuple(part.w_q.shape) == (n, k * bits // 64) and tuple(part.scales.shape) == (n, k // group // 2) and tuple(part.biases.shape) == (n, k // group // 2)
        assert dequantize(part.w_q.view(torch.int32).numpy().view(np.uint32), part.scales, part.biases, bits, group).shape == (n, k // 2)


def test_uqff_shard_contents_and_misaligned(tmp_path):
    w_q, scales, biases, bias = _layer(2, True, bits=3, group=32)  # N 6, K 128: 12 words, 4 groups
    path = str(tmp_path / "s.uqff")
    uqff.write(path, uqff.serialize_afq_layer("l", w_q, scales, biases, 3, 32, bias))
    r = uqff.UqffReader(path)
    d = r.load_afq_layer("l", Shard(dim=1, rank=1, world_size=2))
    assert _eq(d.w_q, w_q[:, 6:].contiguous()) and _eq(d.scales, scales[:, 2:].contiguous()) and _eq(d.biases, biases[:, 2:].contiguous())
    assert d.bias is None and d.bias_mode == "skip"
    d = r.load_afq_layer("l", Shard(dim=1, offset=32, length=64))
    assert _eq(d.w_q, w_q[:, 3:9].contiguous()) and _eq(d.scales, scales[:, 1:3].contiguous())
    with pytest.raises(ValueError, match="Sharding the AFQ packed dim requires group alignment: start 16, len 32, group 32."):
        r.load_afq_layer("l", Shard(dim=1, offset=16, length=32))
    with pytest.raises(ValueError, match="requires group alignment"):
        r.load_afq_layer("l", Shard(dim=1, offset=32, length=48))
    d = r.load_afq_layer("l", Shard(dim=0, rank=1, world_size=3))
    assert _eq(d.w_q, w_q[2:4].contiguous()) and _eq(d.scales, scales[2:4]) and _eq(d.bias, bias[2:4]) and d.bias_mode == "narrow"
    with pytest.raises(ValueError, match="not an AFQ layer|Missing"):
        r.load_afq_layer("nope")


# ------------------------------------------------------------------------------------------------ host mirror
def test_layer_argument_errors():
    w_q, scales, biases, _ = _layer(2, False)
    with pytest.raises(ValueError, match="Invalid AFQ bits 5."):
        afq.AfqLayer.from_parts(w_q, scales, biases, None, 5, 64)
    with pytest.raises(ValueError, match="Invalid AFQ group size 48."):
        afq.AfqLayer.from_parts(w_q, scales, biases, None, 4, 48)
    with pytest.raises(ValueError, match="AFQ weight matrix must be u32"):
        afq.AfqLayer.from_parts(w_q.view(torch.int32).to(torch.uint8), scales, biases, None, 4, 64)
    with pytest.raises(ValueError, match="Scales and biases should have the same shapes"):
        afq.AfqLayer.from_parts(w_q, scales, biases[:, :1], None, 4, 64)
    with pytest.raises(ValueError, match="Last dims of w and scales must be compatible."):
        afq.AfqLayer.from_parts(w_q, scales, biases, None, 8, 64)
    layer = afq.AfqLayer.from_parts(w_q, scales, biases, None, 4, 64)
    with pytest.raises(ValueError, match="must live on the GPU"):
        layer.forward(torch.zeros(1, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="must live on the GPU"):
        afq.quantize_tensors(torch.zeros(2, 64), 4, 64)
    with pytest.raises(ValueError, match="Weight shape mismatch"):
        layer.gather_forward(torch.zeros(1, 128, dtype=torch.bfloat16), torch.zeros(1, 2, dtype=torch.int32))
    tensors = {"p.weight": w_q, "p.scales": scales, "p.biases": biases}
    got = afq.afq_linear_b(128, 6, {"bits": 4, "group_size": 64}, False, tensors, "p")
    assert got.uqff_type() == "AFQ4" and got.in_features == 128 and not got.has_bias()
    with pytest.raises(ValueError, match="shape mismatch for p.weight"):
        afq.afq_linear_b(128, 7, {"bits": 4, "group_size": 64}, False, tensors, "p")
    with pytest.raises(ValueError, match="cannot find tensor p.bias"):
        afq.afq_linear_b(128, 6, {"bits": 4, "group_size": 64}, True, tensors, "p")
    with pytest.raises(ValueError, match="Unexpected quantization config."):
        afq.afq_linear_b(128, 6, {"quant_method": "fp8"}, False, tensors, "p")
    w3, s3, b3, bias3 = _layer(3, True)
    t3 = {"e.weight": w3, "e.scales": s3, "e.biases": b3, "e.bias": bias3}
    got = afq.afq_packed_linear_b(3, 128, 6, {"bits": 4, "group_size": 64}, True, t3, "e")
    assert got.w_q.dim() == 3 and got.has_bias()
    with pytest.raises(ValueError, match="dtype mismatch for e.weight"):
        afq.afq_packed_linear_b(3, 128, 6, {"bits": 4, "group_size": 64}, True, {**t3, "e.weight": w3.view(torch.int32).float()}, "e")


def test_apply_isq_identity_cases():
    """afq/mod.rs:588-619: None and the layer's own type hand back the same object; a stacked layer refuses targets without stacked gather."""
    src = afq.AfqLayer.from_parts(torch.zeros(1, 8, dtype=torch.uint32), torch.zeros(1, 1, dtype=torch.bfloat16), torch.zeros(1, 1, dtype=torch.bfloat16),
                                  torch.zeros(1, dtype=torch.bfloat16), 4, 64)
    assert src.apply_isq(None) is src and src.uqff_type() == "AFQ4" and src.has_bias()
    assert src.apply_isq("AFQ4") is src
    w3, s3, b3, _ = _layer(3, False)
    stacked = afq.AfqLayer.from_parts(w3, s3, b3, None, 4, 64)
    with pytest.raises(ValueError, match="Cannot requantize stacked AFQ expert weights to HQQ4: that target does not support stacked expert gather. "
                                         "Use a Q\\*K/Q\\*_0/Q\\*_1 target, AFQ, or omit ISQ."):
        stacked.apply_isq("HQQ4")
    assert stacked.apply_isq(None) is stacked


# ------------------------------------------------------------------------------------------------ build flags and code objects
def test_build_keeps_division_correctly_rounded():
    """The quantizer's `/` must be IEEE: no fast-math and no opt-out of hipcc's correctly rounded f32 divide (its default) in the build flags."""
    import importlib.util as u
    spec = u.spec_from_file_location("mrs_build_flags", os.path.join(ROOT, "mistral.rs_amd", "build.py"))
    m = u.module_from_spec(spec)
    spec.loader.exec_module(m)
    flags = " ".join(m.CXXFLAGS)
    assert "fast-math" not in flags and "-Ofast" not in flags and "-fno-hip-fp32-correctly-rounded-divide-sqrt" not in flags and "-ffp-contract=off" in flags
    assert "afq.hip" in [t[0] for t in m.libraries()["libmistralrsquant.so"]] and "ext_afq.hip" in [t[0] for t in m.libraries()["libmrs_hip_ext.so"]]


@pytest.mark.parametrize("lib", ["libmistralrsquant.so", "libmrs_hip_ext.so"])
def test_afq_kernels_use_no_scratch(lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    path = os.path.join(ROOT, "mistral.rs_amd", "lib", lib)
    assert os.path.exists(path), f"{lib} is not built"
    ks = [k for k in kernel_resources.resources(path) if "afq" in k["name"] or "afq" in k.get("demangled", "")]
    assert ks, f"no afq kernel in {lib}"
    bad = [(k["demangled"], k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0), k.get("sgpr_spill_count", 0)) for k in ks
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0) or k.get("uses_dynamic_stack", False) is True]
    assert not bad, f"afq kernels with scratch or spills: {bad}"
    # 256-thread workgroups: <= 256 VGPRs keeps one workgroup per CU schedulable at two waves per SIMD... and static LDS stays inside the 64 KiB a kernel may declare
    over = [(k["demangled"], k.get("vgpr_count", 0), k.get("group_segment_fixed_size", 0)) for k in ks
            if k.get("vgpr_count", 0) > 256 or k.get("group_segment_fixed_size", 0) > 64 * 1024]
    assert not over, f"afq kernels over 256 VGPRs or 64 KiB of static LDS: {over}"
