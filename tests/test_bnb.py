"""CPU: bitsandbytes NF4 / FP4 -- a numpy oracle written from the contract of DESIGN 4.19 (the GPU file imports it), nibble and quant_state packers, the
loader's errors (each raised before any device call) and an f32 restatement of "decode, then a k-ordered chain" held to the bound of the GPU tests:

    |got - E| <= B (1 + u) + u |E|,   B = 2 (K + 4) 2^-24 (sum_k |x_k| |W_kn| + |bias_n|),   u = 2^-8 (bf16), 2^-11 (f16), 0 (f32)

with E the f64 value at the oracle's W_hat (the derivation is that of tests/test_zz_gptq_gpu.py: W_hat is already rounded, a product of two T values is exact
in f32 for 16-bit T and costs one more rounding for f32, within the K + 4).  The GPU side is tests/test_zz_bnb_gpu.py."""
import json

import numpy as np
import pytest
import torch

import mistralrs_amd  # noqa: F401
from mistralrs_amd import bnb

TABLES = {"nf4": np.array(bnb.NF4_TABLE, np.float32), "fp4": np.array(bnb.FP4_TABLE, np.float32)}
UNIT = {"float32": 0.0, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
T_MAX = {"float32": float(np.finfo(np.float32).max), "float16": 65504.0, "bfloat16": float(np.float32(2.0 ** 127) * np.float32(2 - 2.0 ** -7))}


# ------------------------------------------------------------------------------------------------ oracle
def rne(v32, dtype):
    """f32 -> T by round-to-nearest-even, returned as (f32 values, bit pattern)"""
    v32 = np.ascontiguousarray(v32, dtype=np.float32)
    if dtype == "float32":
        return v32, v32.view(np.int32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            h = v32.astype(np.float16)
        return h.astype(np.float32), h.view(np.int16)
    b = v32.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint32)  # finite inputs only
    return (b << 16).view(np.float32), b.astype(np.uint16).view(np.int16)


def absmax_f32(absmax, nested=None):
    """A_b: plain f32, or f32(f32(nested_quant_map[absmax[b]] * nested_absmax[b // nested_blocksize]) + f32(nested_offset))"""
    if nested is None:
        return np.asarray(absmax, np.float32)
    nabs, nqm, nbs, off = nested
    prod = nqm[absmax].astype(np.float32) * nabs[np.arange(len(absmax)) // nbs].astype(np.float32)
    return (prod.astype(np.float32) + np.float32(off)).astype(np.float32)


def dequantize(codes, table, absmax, blocksize, dtype, nested=None):
    """W_hat of flat codes: RNE_T(f32(table[q] * A_{i // blocksize}))"""
    a = absmax_f32(absmax, nested)[np.arange(len(codes)) // blocksize]
    return rne(np.asarray(table, np.float32)[codes] * a, dtype)


def pack_nibbles(codes):
    """flat 4-bit codes -> (n + 1) // 2 bytes, element 2 i in the high nibble"""
    c = np.concatenate([np.asarray(codes, np.uint8), np.zeros(len(codes) & 1, np.uint8)])
    return ((c[0::2] << 4) | c[1::2]).astype(np.uint8)


def pack_state(**fields):
    return torch.tensor(list(json.dumps(fields).encode()), dtype=torch.uint8)


def check_bound(got, exact, mag, k, dtype, what):
    u = UNIT[dtype]
    b = 2.0 * (k + 4) * 2.0 ** -24 * mag
    assert float((np.abs(exact) + b).max()) < T_MAX[dtype], what  # nothing near the overflow threshold
    lim = b * (1 + u) + u * np.abs(exact)
    err = np.abs(got.astype(np.float64) - exact)
    print(f"{what}: worst error / bound = {float(np.max(err / np.maximum(lim, 1e-300))):.3f}")
    bad = np.argwhere(~(err <= lim))
    assert not len(bad), f"{what}: {len(bad)} of {err.size} elements outside the bound; first at {tuple(bad[0])}"


# ------------------------------------------------------------------------------------------------ tests
def checkpoint(rng, qt="nf4", n=3, k=64, blocksize=64, nested=True, dtype="bfloat16"):
    blocks = -(-n * k // blocksize)
    codes = rng.integers(0, 16, n * k).astype(np.uint8)
    t = {"m.weight": torch.from_numpy(pack_nibbles(codes)).reshape(-1, 1), "m.weight.quant_map": bnb.table(qt), "m.bias": torch.zeros(n)}
    state = dict(blocksize=blocksize, shape=[n, k], dtype=dtype, quant_type=qt)
    if nested:
        state.update(nested_blocksize=256, nested_offset=0.02, nested_dtype="float32")
        t["m.weight.absmax"] = torch.from_numpy(rng.integers(0, 256, blocks).astype(np.uint8))
        t["m.weight.nested_absmax"] = torch.full((-(-blocks // 256),), 0.01)
        t["m.weight.nested_quant_map"] = torch.linspace(-1, 1, 256)
    else:
        t["m.weight.absmax"] = torch.from_numpy(rng.uniform(0.01, 0.1, blocks).astype(np.float32))
    t[f"m.weight.quant_state.bitsandbytes__{qt}"] = pack_state(**state)
    return t, state


def restate(t, state, qt="nf4"):
    t[f"m.weight.quant_state.bitsandbytes__{qt}"] = pack_state(**state)


def test_tables_and_packer():
    assert np.signbit(TABLES["fp4"][8]) and TABLES["fp4"][8] == 0 and TABLES["fp4"][9] == np.float32(-5.208333333e-03)
    assert (np.diff(TABLES["nf4"]) > 0).all() and TABLES["nf4"][7] == 0 and TABLES["nf4"][[0, 15]].tolist() == [-1, 1]
    assert pack_nibbles([1, 2, 3]).tolist() == [0x12, 0x30]


def test_loader_builds_a_layer_and_refuses_the_cpu():
    rng = np.random.default_rng(0)
    for qt, nested in (("nf4", True), ("fp4", False)):
        t, _ = checkpoint(rng, qt, nested=nested)
        layer = bnb.bnb_linear_b(64, 3, True, t, "m")
        assert (layer.name(), layer.quant_type, layer.has_bias(), layer.isq_serde_supported(), layer.quantized_act_type()) == ("bnb-linear", qt, True, False, None)
        assert layer.dtype_and_device()[0] == torch.bfloat16 and (layer.nested_absmax is not None) == nested
        with pytest.raises(ValueError, match="must live on the GPU"):
            layer.forward(torch.zeros(1, 64))
        with pytest.raises(ValueError, match="does not support `gather_forward`"):
            layer.gather_forward(None, None)
        with pytest.raises(ValueError, match="does not support adding weight delta"):
            layer.add_delta_w(None)


def test_loader_errors():
    rng = np.random.default_rng(1)
    load = lambda t, i=64, o=3: bnb.bnb_linear_b(i, o, False, t, "m")
    t, state = checkpoint(rng)
    with pytest.raises(ValueError, match="this means the layer is not 4bit"):
        load({k: v for k, v in t.items() if "quant_state" not in k})
    restate(t, dict(state, blocksize=32))
    with pytest.raises(ValueError, match=r"Blocksize of 32 is not supported, \[2048, 4096, 1024, 512, 256, 128, 64\] are"):
        load(t)
    restate(t, state)
    with pytest.raises(ValueError, match="shape mismatch"):
        load(t, 32, 6)
    with pytest.raises(ValueError, match="bytes, expected 96"):
        load(dict(t, **{"m.weight": t["m.weight"][:-1]}))
    with pytest.raises(ValueError, match="absmax has 2 entries, expected 3"):
        load(dict(t, **{"m.weight.absmax": t["m.weight.absmax"][:2]}))
    restate(t, {k: v for k, v in state.items() if k != "nested_blocksize"})
    with pytest.raises(ValueError, match="`nested_blocksize` must be present"):
        load(t)
    restate(t, state)
    qm = bnb.table("nf4")
    qm[3] = float(np.nextafter(np.float32(qm[3]), np.float32(1)))  # one ulp
    with pytest.raises(ValueError, match="differs from the built-in nf4 table"):
        load(dict(t, **{"m.weight.quant_map": qm}))
    assert load(t).blocksize == 64  # the untouched checkpoint loads


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_decode_then_k_ordered_chain_is_inside_the_bound(dtype):
    rng = np.random.default_rng(2)
    m, n, k, bs = 3, 5, 192, 64
    codes = rng.integers(0, 16, n * k)
    nested = (rng.uniform(0.005, 0.02, 1).astype(np.float32), np.sort(rng.uniform(-1, 1, 256)).astype(np.float32), 256, 0.02)
    w = dequantize(codes, TABLES["nf4"], rng.integers(0, 256, n * k // bs), bs, dtype, nested)[0].reshape(n, k).astype(np.float64)
    x = rne(rng.standard_normal((m, k)), dtype)[0].astype(np.float64)
    bias = rne(rng.uniform(-1, 1, n), dtype)[0].astype(np.float64)
    acc = np.zeros((m, n), np.float32)
    for kk in range(k):  # f32 product (exact for 16-bit T), f32 add
        acc = acc + (x[:, kk:kk + 1] * w[:, kk]).astype(np.float32)
    got = rne(acc + bias.astype(np.float32), dtype)[0]
    check_bound(got, x @ w.T + bias, np.abs(x) @ np.abs(w.T) + np.abs(bias), k, dtype, f"chain {dtype}")
