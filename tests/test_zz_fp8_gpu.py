"""GPU: the per-tensor FP8 kernels (scalar conversions, dynamic / static quantizer, dequantize and row gather, the W8A8 matmul on every route) and the two layers
against the numpy oracle of tests/test_fp8.py, written from the contract of DESIGN 4.18: bytes decoded exactly, f64 sums.  Conversions, quantizers, dequantize and
the exact-data matmuls are compared bit for bit; random matmuls are held, element by element and with no exclusions, to

    |out - E| <= B (1 + u_T) + u_T |E|,   B = 2 (K + 4) 2^-24 sum |xq wq| dq_x dq_w + 2^-24 |bias| + C

with the f16 overflow and subnormal allowances of check_bound in tests/test_zz_blockwise_fp8_gpu.py.  C is 0 on route 3 (plain f32 fma, no matrix core): the issue's
bound as written.  On routes 1 and 2, C is what the FP8 matrix core does, measured on the device (scripts/probe_fp8_mfma.py, profiles/fp8.md): inside
one v_mfma_*_fp8_fp8 every product is cut toward zero onto the grid 2^(e - 13), e the exponent of the instruction's largest product, so an instruction of g products
is off by less than (g - 1) 2^-13 times its largest one; C is that, summed over the instructions of the dot product as the kernels form them (mfma_cut below).
Without C random bytes on route 2 at K = 176, bf16 reached 2.08 times the bound in 28 of 19760 elements; products that lie on the grid (the exact cases) are untouched."""
import numpy as np
import pytest
import torch

import mistralrs_amd  # noqa: F401
from mistralrs_amd import fp8
from mistralrs_amd.blockwise_fp8 import BlockwiseFP8Linear
from tests.test_blockwise_fp8 import e4m3_decode
from tests.test_fp8 import encode, quant_dynamic_oracle, quant_static_oracle
from tests.test_zz_blockwise_fp8_gpu import EXACT_CODES, bits, check_bound, gpu, to_t

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
ALL3 = [torch.float32, torch.float16, torch.bfloat16]
ids_of = lambda ts: [str(t).split(".")[-1] for t in ts]
LUT = e4m3_decode(np.arange(256, dtype=np.uint8))  # f64, NaN at 0x7f / 0xff
FINITE = np.array([b for b in range(256) if b & 0x7F != 0x7F], dtype=np.uint8)
TILE = 128  # route 2's tile edge in M, N and K; route 1 takes M <= 16 and stages 4096 k at a time


def f32_of(t):
    return t.detach().float().cpu().numpy()


def random_bytes(rng, *shape):
    return FINITE[rng.integers(0, len(FINITE), shape)]


def random_values(rng, n, dtype):
    """normal values with a few large ones, rounded to dtype"""
    v = rng.standard_normal(n) * np.exp(rng.uniform(-6, 3, n))
    v[rng.integers(0, n, max(1, n // 50))] *= 100.0
    return to_t(v, dtype)


# ------------------------------------------------------------------------------------------------ scalar conversions
@pytest.mark.parametrize("dtype", ALL3, ids=ids_of(ALL3))
def test_scalar_conversions(dtype):
    codes = np.arange(256, dtype=np.uint8)
    got = f32_of(fp8.fp8_to_dtype(gpu(codes), dtype)).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(LUT)) and np.array_equal(got[~np.isnan(LUT)], LUT[~np.isnan(LUT)])
    assert np.array_equal(np.signbit(got[~np.isnan(LUT)]), np.signbit(LUT[~np.isnan(LUT)]))
    # every code, every midpoint between neighbours (a tie), both sides of each tie, the saturation edge, and (f32 only) values whose f16 rounding lands on a tie
    grid = np.sort(LUT[FINITE])
    mids = (grid[:-1] + grid[1:]) / 2
    vals = np.concatenate([grid, mids, mids * (1 + 2.0 ** -7), mids * (1 - 2.0 ** -7), mids * (1 + 2.0 ** -12), mids * (1 - 2.0 ** -12),
                           [448.0, 449.0, 463.9, 464.0, 465.0, 480.0, 1e4, -1e4, 2.0 ** -10, 2.0 ** -11, -0.0]])
    src = to_t(vals, dtype)
    assert np.array_equal(fp8.dtype_to_fp8(src.to("cuda")).cpu().numpy(), encode(f32_of(src)))


# ------------------------------------------------------------------------------------------------ quantizers
# 17 / 4099: not a multiple of the 16 elements of a lane, one workgroup; 32768 + 5: the staged path, several workgroups; 4.2 M + 3: more units than the grid's cap
@pytest.mark.parametrize("dtype,n", [(t, n) for t in ALL3 for n in (1, 17, 4099, 32768 + 5)] + [(torch.bfloat16, 4_200_003)])
def test_quantizers(dtype, n):
    x = random_values(np.random.default_rng(n), n, dtype)
    q, s, dq = fp8.quantize_tensor(x.to("cuda"))
    wq, ws, wdq = quant_dynamic_oracle(f32_of(x))
    assert bits(s)[0] == ws.view(np.int32) and bits(dq)[0] == wdq.view(np.int32), (float(s), float(ws), float(dq), float(wdq))
    assert np.array_equal(q.cpu().numpy(), wq)
    if n <= 100_000:
        scale = torch.tensor(0.37, device="cuda")
        assert np.array_equal(fp8.quantize_static(x.to("cuda"), scale).cpu().numpy(), quant_static_oracle(f32_of(x), np.float32(0.37)))
    if n == 17:  # amax == 0, and a tensor whose amax is below 1
        for z in (torch.zeros(n, dtype=dtype), x * 0 + 0.25):
            q, s, dq = fp8.quantize_tensor(z.to("cuda"))
            wq, ws, wdq = quant_dynamic_oracle(f32_of(z))
            assert float(s) == 448.0 == float(ws) and bits(dq)[0] == wdq.view(np.int32) and np.array_equal(q.cpu().numpy(), wq)


# ------------------------------------------------------------------------------------------------ dequantize, row gather
@pytest.mark.parametrize("shape", [(37, 48), (5, 19)], ids=["vector", "bytewise"])
@pytest.mark.parametrize("dtype", ALL3, ids=ids_of(ALL3))
def test_dequantize_and_gather(dtype, shape):
    rng = np.random.default_rng(shape[1])
    w, scale = random_bytes(rng, *shape), np.float32(0.0123)
    want = lambda rows: to_t(LUT[w[rows]].astype(np.float32) * scale, dtype)  # one f32 product, one rounding
    sc = torch.tensor(float(scale), device="cuda")
    assert np.array_equal(bits(fp8.dequantize(gpu(w), sc, dtype)), bits(want(slice(None))))
    ids = np.array([[shape[0] - 1, 0, 3], [3, 3, 1]])
    got = fp8.dequantize(gpu(w), sc, dtype, gpu(ids))
    assert tuple(got.shape) == (2, 3, shape[1]) and np.array_equal(bits(got), bits(want(ids)))
    with pytest.raises(ValueError, match=f"index {shape[0]} is out of bounds for {shape[0]} rows"):
        fp8.dequantize(gpu(w), sc, dtype, gpu(np.array([0, shape[0]])))
    layer = fp8.FP8Linear.from_parts(gpu(w), None, sc, sc, sc)
    assert np.array_equal(bits(layer.embedding_forward(gpu(ids))), bits(to_t(LUT[w[ids]].astype(np.float32) * scale, torch.float32)))


# ------------------------------------------------------------------------------------------------ matmul, exact data
def exact_codes(rows, k, salt):
    """small integers and halves, a pattern asymmetric in the row, in k and between the two operands"""
    r, kk = np.arange(rows)[:, None], np.arange(k)[None, :]
    return EXACT_CODES[(3 * r + 5 * kk + (r * kk) // 7 + salt) % len(EXACT_CODES)]


def run_matmul(xq, wq, dqx, dqw, bias, dtype, view_offset=0):
    """returns (out as f64, exact f64 result, sum |xq wq| dq_x dq_w)"""
    dx, dw = gpu(np.float32([dqx])), gpu(np.float32([dqw]))
    xg = gpu(xq)
    if view_offset:  # the same bytes at an address that is not a multiple of 16
        buf = torch.zeros(xq.size + 16, dtype=torch.uint8, device="cuda")
        xg = buf[view_offset:view_offset + xq.size].view(xq.shape).copy_(xg)
    out = fp8.matmul_q(xg, gpu(wq), dx, dw, None if bias is None else to_t(bias, dtype).to("cuda"), dtype)
    a, b, sc = LUT[xq], LUT[wq], float(np.float32(dqx)) * float(np.float32(dqw))
    exact = (a @ b.T) * sc + (0.0 if bias is None else f32_of(to_t(bias, dtype)).astype(np.float64))
    return out, exact, (np.abs(a) @ np.abs(b).T) * sc


# N: 16, not a multiple of 16, one tile plus an edge.  K: one MFMA step, a multiple of 16 but not of the tile's 128, across route 1's 4096-k LDS chunk
@pytest.mark.parametrize("n,k", [(16, 32), (40, 48), (TILE + 24, 4096 + 64)])
@pytest.mark.parametrize("m", [1, 15, 16, 17, TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of(DTYPES))
def test_matmul_exact(dtype, m, n, k):
    bias = (np.arange(n) % 7 - 3).astype(np.float64)
    out, exact, _ = run_matmul(exact_codes(m, k, 0), exact_codes(n, k, 4), 0.5, 0.25, bias, dtype)
    assert fp8.fp8_pertensor_last_route() == (1 if m <= 16 else 2)
    assert np.array_equal(bits(out), bits(to_t(exact, dtype)))  # every partial sum is an exact f32: RNE_T(exact) on every route


@pytest.mark.parametrize("m,k,offset", [(3, 48, 1), (20, 48, 1), (3, 40, 0), (20, 40, 0)], ids=["unaligned-3", "unaligned-20", "k40-3", "k40-20"])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of(DTYPES))
def test_matmul_exact_general_route(dtype, m, k, offset):
    out, exact, _ = run_matmul(exact_codes(m, k, 0), exact_codes(21, k, 4), 2.0, 0.5, None, dtype, offset)
    assert fp8.fp8_pertensor_last_route() == 3 and np.array_equal(bits(out), bits(to_t(exact, dtype)))


def test_route1_row_does_not_depend_on_m():
    rng = np.random.default_rng(5)
    xq, wq = random_bytes(rng, 16, 4096 + 64), random_bytes(rng, 40, 4096 + 64)
    full, _, _ = run_matmul(xq, wq, 0.01, 0.02, None, torch.bfloat16)
    for r in (0, 7, 15):
        one, _, _ = run_matmul(xq[r:r + 1], wq, 0.01, 0.02, None, torch.bfloat16)
        assert fp8.fp8_pertensor_last_route() == 1 and np.array_equal(bits(one)[0], bits(full)[r])


# ------------------------------------------------------------------------------------------------ matmul and layers, bounded
def mfma_cut(xq, wq, sc, route):
    """C of the docstring.  Route 1 puts the k of one 64-k block that share (k % 16) // 8 into one instruction (g = 32), route 2 those of a 32-k block (g = 16)."""
    if route == 3:
        return 0.0
    blk, (m, k), n = (64 if route == 1 else 32), xq.shape, wq.shape[0]
    p = np.pad(np.abs(LUT[xq])[:, None, :] * np.abs(LUT[wq])[None, :, :], ((0, 0), (0, 0), (0, -k % blk))).reshape(m, n, -1, blk // 16, 2, 8)
    return (blk // 2 - 1) * 2.0 ** -13 * p.max(axis=(3, 5)).sum(axis=(2, 3)) * sc


def bounded(out, exact, mag, k, dtype, what, bias=None, cut=0.0):
    """check_bound holds got to 2 (K + 4) 2^-24 mag: B's other two terms are folded into mag"""
    mag = mag + (cut * 2.0 ** 24 + (0.0 if bias is None else np.abs(bias))) / (2.0 * (k + 4))
    check_bound(f32_of(out).reshape(exact.shape), exact, mag, k, dtype, what)


@pytest.mark.parametrize("m,n,k,route", [(5, 72, 4096 + 64, 1), (TILE + 2, TILE + 24, 176, 2), (3, 20, 40, 3)], ids=["route1", "route2", "route3"])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of(DTYPES))
def test_matmul_random_bound(dtype, m, n, k, route):
    rng = np.random.default_rng(k)
    dqx, dqw, bias = np.float32(rng.uniform(1e-3, 1e-2)), np.float32(rng.uniform(1e-3, 1e-2)), rng.standard_normal(n)
    bias = f32_of(to_t(bias, dtype)).astype(np.float64)
    xq, wq = random_bytes(rng, m, k), random_bytes(rng, n, k)
    out, exact, mag = run_matmul(xq, wq, dqx, dqw, bias, dtype)
    assert fp8.fp8_pertensor_last_route() == route
    bounded(out, exact, mag, k, dtype, f"matmul_q route {route} {dtype}", bias, mfma_cut(xq, wq, float(dqx) * float(dqw), route))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of(DTYPES))
def test_fp8_linear_end_to_end(dtype, with_bias):
    rng = np.random.default_rng(11)
    n, k = 72, 176
    w, x = random_values(rng, n * k, torch.float32).reshape(n, k), random_values(rng, 2 * 9 * k, dtype).reshape(2, 9, k)  # rank 3: 18 rows, route 2
    bias = to_t(rng.standard_normal(n), dtype) if with_bias else None
    layer = fp8.FP8Linear.quantize(w.to("cuda"), None if bias is None else bias.to("cuda"))
    wq, ws, wdq = quant_dynamic_oracle(f32_of(w))
    assert np.array_equal(layer.weight.cpu().numpy(), wq) and bits(layer.quant_scale)[0] == ws.view(np.int32) and bits(layer.dequant_w_scale)[0] == wdq.view(np.int32)
    assert np.array_equal(bits(layer.dequantize_w()), bits(to_t(LUT[wq].astype(np.float32) * wdq, torch.float32)))
    y = layer.forward(x.to("cuda"))
    assert tuple(y.shape) == (2, 9, n) and y.dtype == dtype and fp8.fp8_pertensor_last_route() == 2
    xq, _, xdq = quant_dynamic_oracle(f32_of(x).reshape(-1, k))
    b64 = None if bias is None else f32_of(bias).astype(np.float64)
    sc = float(xdq) * float(wdq)
    bounded(y, (LUT[xq] @ LUT[wq].T) * sc + (0.0 if b64 is None else b64), (np.abs(LUT[xq]) @ np.abs(LUT[wq]).T) * sc, k, dtype, f"FP8Linear {dtype}", b64,
            mfma_cut(xq, wq, sc, 2))
    grown = layer.add_delta_w(torch.ones(n, k, device="cuda"))  # dequantize, add, requantize
    assert np.array_equal(grown.weight.cpu().numpy(), quant_dynamic_oracle(LUT[wq].astype(np.float32) * wdq + np.float32(1.0))[0])
    assert isinstance(fp8.PerTensorFP8Linear(layer.weight, layer.dequant_w_scale).apply_isq("F8E4M3"), fp8.FP8Linear)


@pytest.mark.parametrize("act_quant", ["none", "static", "dynamic"])
def test_pertensor_fp8_linear_modes(act_quant):
    rng = np.random.default_rng(13)
    n, k, dtype = 40, 176, torch.bfloat16
    wq, scale_inv, act = random_bytes(rng, n, k), np.float32(0.004), np.float32(0.031)
    x, bias = random_values(rng, 5 * k, dtype).reshape(5, k), to_t(rng.standard_normal(n), dtype)
    tensors = {"p.weight": gpu(wq), "p.weight_scale_inv": gpu(np.float32([scale_inv]))[0], "p.activation_scale": gpu(np.float32([act]))[0], "p.bias": bias.to("cuda")}
    layer = fp8.pertensor_fp8_linear_b(k, n, True, tensors, "p", act_quant=act_quant)
    assert np.array_equal(bits(layer.dequantize_w()), bits(to_t(LUT[wq].astype(np.float32) * scale_inv, dtype)))
    y = layer.forward(x.to("cuda"))
    b64 = f32_of(bias).astype(np.float64)
    if act_quant == "none":  # weight-only: the blockwise layer (tests/test_zz_blockwise_fp8_gpu.py) with one block over the whole weight, bit for bit
        same = BlockwiseFP8Linear(gpu(wq), gpu(np.float32([[scale_inv]])), bias.to("cuda"), dtype, (n, k))
        assert np.array_equal(bits(y), bits(same.forward(x.to("cuda"))))
        return
    xq, xdq = (quant_static_oracle(f32_of(x), act), act) if act_quant == "static" else quant_dynamic_oracle(f32_of(x))[::2]
    sc = float(xdq) * float(scale_inv)
    bounded(y, (LUT[xq] @ LUT[wq].T) * sc + b64, (np.abs(LUT[xq]) @ np.abs(LUT[wq]).T) * sc, k, dtype,
            f"PerTensorFP8Linear {act_quant}", b64, mfma_cut(xq, wq, sc, 1))
