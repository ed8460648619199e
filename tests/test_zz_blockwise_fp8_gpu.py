"""GPU: the blockwise-FP8 kernels (dequantize, quantize, dense matmul on every route, MoE gather) and `BlockwiseFP8Linear` against a numpy oracle written from
the format definition (tests/test_blockwise_fp8.py pins its E4M3 rounding against torch): weights decoded exactly, f64 sums.  Dequantize and quantize are
compared bit for bit, and so are the exact-integer matmul cases; random cases are held, element by element and with no exclusions, to

    |out - exact| <= B (1 + u_T) + u_T |exact|,   B = 2 (K + 4) 2^-24 sum |x_k w_k s|,   u_T = 2^-8 (bf16) / 2^-11 (f16)

((K + 4) 2^-24 sum |x w s| bounds K - 1 round-to-nearest f32 additions plus the scale multiply in any order; the factor 2 covers a truncating adder in the
matrix core; u_T |exact| is the one rounding to T).  f16 results past 65520 must be the infinity of their sign, and results below 2^-14 sit on the fixed 2^-24
grid where one rounding is off by up to 2^-25, as in tests/test_zz_mxfp4_gpu.py."""
import numpy as np
import pytest
import torch

import mistralrs_amd  # noqa: F401
from mistralrs_amd import blockwise_fp8 as bf8
from mistralrs_amd.distributed import Shard
from tests.test_blockwise_fp8 import e4m3_decode, e4m3_encode_f16, quant_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
ALL3 = [torch.float32, torch.float16, torch.bfloat16]
LUT = e4m3_decode(np.arange(256, dtype=np.uint8))  # f64, NaN at 0x7f / 0xff
F16_OVERFLOW = 65520.0  # round-to-nearest-even gives inf from here on
GEOMETRIES = [(128, 128), (2, 64), (3, 48)]


# ------------------------------------------------------------------------------------------------ oracle
def expand(scale, n, k, bs):
    """scale [.., gy, >= gx] -> the scale of every element [.., n, k]"""
    return np.repeat(np.repeat(scale, bs[0], -2), bs[1], -1)[..., :n, :k]


def dequant_f64(w, scale, bs):
    return LUT[w] * expand(scale.astype(np.float64), w.shape[-2], w.shape[-1], bs)


def dequant_f32(w, scale, bs):
    with np.errstate(invalid="ignore"):
        return LUT[w].astype(np.float32) * expand(scale.astype(np.float32), w.shape[-2], w.shape[-1], bs)  # one f32 product


def to_t(a, dtype):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_bound(got, exact, mag, k, dtype, what):
    u = U[dtype]
    b = 2.0 * (k + 4) * 2.0 ** -24 * mag
    got = got.astype(np.float64)
    lim = b * (1 + u) + u * np.abs(exact)
    if dtype == torch.float16:
        lim = lim + np.where(np.abs(exact) < 2.0 ** -14 + b, 2.0 ** -25, 0.0)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - exact) <= lim
    if dtype == torch.float16:
        inf_ok = np.isinf(got) & (np.sign(got) == np.sign(exact))
        must, may = np.abs(exact) - b >= F16_OVERFLOW, np.abs(exact) + b >= F16_OVERFLOW
        ok = np.where(must, inf_ok, np.where(may, ok | inf_ok, ok))
    fin = np.isfinite(got)
    worst = float(np.max(np.abs(got - exact)[fin] / np.maximum(lim[fin], 1e-300))) if fin.any() else 0.0
    print(f"{what}: worst error / bound = {worst:.3f}")
    bad = np.argwhere(~ok)
    assert not len(bad), (f"{what}: {len(bad)} of {ok.size} elements outside the bound (worst finite {worst:.2f}x); first at {tuple(bad[0])}: "
                          f"got {got[tuple(bad[0])]!r} exact {exact[tuple(bad[0])]!r} bound {lim[tuple(bad[0])]!r}")


EXACT_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0])
EXACT_CODES = e4m3_encode_f16(EXACT_VALUES.astype(np.float16))


def exact_weights(n, k, e=0):
    """small integers and halves, a pattern asymmetric in n and k"""
    nn, kk = np.arange(n)[:, None], np.arange(k)[None, :]
    return EXACT_CODES[(3 * nn + 5 * kk + (nn * kk) // 7 + 11 * e) % len(EXACT_CODES)]


def exact_scales(n, k, bs, pad=0, e=0):
    gy, gx = -(-n // bs[0]), -(-k // bs[1])
    i, j = np.arange(gy)[:, None], np.arange(gx + pad)[None, :]
    s = (2.0 ** ((3 * i + j + e) % 3 - 1)).astype(np.float32)
    s[:, gx:] = np.nan  # padding columns are never read
    return s


def random_weights(rng, *shape):
    w = rng.integers(0, 256, shape, dtype=np.uint8)
    w[(w & 0x7F) == 0x7F] = 0x7E  # every byte except the NaNs
    return w


def random_scales(rng, shape, bs, pad=0):
    gy, gx = -(-shape[-2] // bs[0]), -(-shape[-1] // bs[1])
    s = (2.0 ** rng.integers(-6, -1, (*shape[:-2], gy, gx + pad)) * rng.uniform(1.0, 2.0, (*shape[:-2], gy, gx + pad))).astype(np.float32)
    s[..., gx:] = np.nan
    return s


def off_by_one_element(t):
    """the same values at an address that is aligned to the element only"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 4 == 2 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------ dequantize
@pytest.mark.parametrize("dtype", ALL3, ids=["f32", "f16", "bf16"])
def test_dequantize_every_byte(dtype):
    scales = np.array([[2.0 ** -20], [0.37], [1.0], [3e4]], np.float32)
    w = np.tile(np.arange(256, dtype=np.uint8), (4, 1))
    want32 = dequant_f32(w, scales, (1, 256))
    got = bf8.dequantize(gpu(w), gpu(scales), (1, 256), dtype).cpu()
    nan = np.isnan(want32)
    assert nan.sum() == 8 and np.array_equal(torch.isnan(got).numpy(), nan)
    want = torch.from_numpy(want32).to(dtype)  # one conversion from the f32 product
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])  # subnormals, signed zeros, f16 overflow to inf included


@pytest.mark.parametrize("bs", GEOMETRIES, ids=str)
def test_dequantize_geometries(bs):
    rng = np.random.default_rng(1)
    w = rng.integers(0, 256, (5, 200), dtype=np.uint8)
    s = random_scales(rng, (5, 200), bs, pad=1)  # scale_stride = columns + 1
    want32 = dequant_f32(w, s, bs)
    nan = np.isnan(want32)
    for dtype in ALL3:
        got = bf8.dequantize(gpu(w), gpu(s), bs, dtype).cpu()
        assert np.array_equal(torch.isnan(got).numpy(), nan)
        assert np.array_equal(bits(got)[~nan], bits(torch.from_numpy(want32).to(dtype))[~nan])
    # the layer over float8_e4m3fn storage, stacked experts
    s2 = np.ascontiguousarray(np.stack([s[:, :-1], s[:, :-1] * 2]))
    layer = bf8.blockwise_fp8_moe(gpu(np.stack([w, w])).view(torch.float8_e4m3fn), gpu(s2), bs, dequant_dtype=torch.float16)
    got = layer.dequantize_w().cpu()
    want = torch.from_numpy(dequant_f32(np.stack([w, w]), s2, bs)).to(torch.float16)
    assert tuple(got.shape) == (2, 5, 200) and np.array_equal(bits(got)[~np.stack([nan, nan])], bits(want)[~np.stack([nan, nan])])


# ------------------------------------------------------------------------------------------------ quantize
def quant_input(rng):
    w = (rng.standard_normal((5, 200)) * 3.0).astype(np.float32)
    w[0, 0], w[0, 1] = 448.0, 1.0625 + 2.0 ** -13       # with (128, 128): scale == 1; f32 -> f16 drops the 2^-13, then the tie goes to the even 1.0 (0x38)
    w[0, 2:8] = [1.0625, 1.1875, 17.0, -17.0, 1.5 * 2.0 ** -9, -2.5 * 2.0 ** -9]  # E4M3 ties, normal and subnormal
    w[1, 0], w[1, 1] = -448.0, 447.9
    w[:, 128:] = 0.0                                     # with (128, 128): an all-zero block
    w[2, 130], w[4, 199] = -0.0, -0.0
    return w


@pytest.mark.parametrize("dtype", ALL3, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("bs", GEOMETRIES, ids=str)
def test_quantize_bit_exact(bs, dtype):
    w = torch.from_numpy(quant_input(np.random.default_rng(2))).to(dtype)
    want_q, want_s = quant_oracle(w.float().numpy(), *bs)
    gx = want_s.shape[1]
    q, s = bf8.quantize_tensors(w.to(DEV), bs, scale_row_stride=gx + 1)
    q, s = q.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(s[:, :gx].view(np.int32), want_s.view(np.int32)) and not s[:, gx].any()
    bad = np.argwhere(q != want_q)
    assert not len(bad), f"{len(bad)} bytes differ; first at {tuple(bad[0])}: got {q[tuple(bad[0])]:#x} want {want_q[tuple(bad[0])]:#x} for {w[tuple(bad[0])]!r}"
    if bs == (128, 128):
        assert s[0, 0] == 1.0 and q[0, 0] == 0x7E and q[1, 0] == 0xFE
        assert s[0, 1] == np.float32(1e-12) and q[2, 130] == 0x80 and q[4, 199] == 0x80 and not (q[:, 128:] & 0x7F).any()
        if dtype == torch.float32:
            assert q[0, 1] == 0x38  # the double-rounding pin: a single rounding of 1.0625 + 2^-13 gives 0x39


# ------------------------------------------------------------------------------------------------ dense
SHAPES = [(1, 40), (3, 72), (8, 136), (9, 136), (33, 200), (70, 136), (130, 72)]
KS = [128, 160, 384]
BLOCKS = [(128, 128), (16, 32)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("bs", BLOCKS, ids=str)
def test_dense_exact_integer(bs, dtype):
    rng = np.random.default_rng(3)
    for k in KS:
        pad = 1 if k == 160 else 0  # scale_row_stride padded by one
        for m, n in SHAPES:
            w, s = exact_weights(n, k), exact_scales(n, k, bs, pad)
            x = rng.integers(-2, 3, (m, k)).astype(np.float64)
            exact = x @ dequant_f64(w, s, bs).T
            got = bf8.matmul(to_t(x, dtype).to(DEV), gpu(w), gpu(s), bs)
            assert bf8.last_route() == (1 if m <= 8 else 2), (m, bf8.last_route())
            assert np.array_equal(bits(got), bits(to_t(exact, dtype))), f"M {m} N {n} K {k} blocks {bs}: differs from the correctly rounded exact result"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("bs", BLOCKS, ids=str)
def test_dense_random(bs, dtype):
    rng = np.random.default_rng(4)
    for k in KS + [2176]:  # 2176 > the GEMV's 2048-k staging chunk
        pad = 1 if k == 160 else 0
        for m, n in (SHAPES if k != 2176 else [(1, 40), (8, 136), (9, 136)]):
            w, s = random_weights(rng, n, k), random_scales(rng, (n, k), bs, pad)
            wd = dequant_f64(w, s, bs)
            tx = to_t(rng.standard_normal((m, k)), dtype).to(DEV)
            if m in (3, 33):
                tx = off_by_one_element(tx)
            x = tx.double().cpu().numpy()
            got = bf8.matmul(tx, gpu(w), gpu(s), bs)
            assert bf8.last_route() == (1 if m <= 8 else 2), (m, bf8.last_route())
            check_bound(got.float().cpu().numpy(), x @ wd.T, np.abs(x) @ np.abs(wd).T, k, dtype, f"dense M {m} N {n} K {k} blocks {bs}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dense_general_route(dtype):
    """K % 16 != 0 and a block width that is no multiple of 16: the general kernel, with x at a 2-byte aligned address."""
    rng = np.random.default_rng(5)
    k, bs = 100, (3, 48)
    for m, n in [(1, 40), (9, 72), (33, 7)]:
        w, s = random_weights(rng, n, k), random_scales(rng, (n, k), bs, pad=1)
        wd = dequant_f64(w, s, bs)
        tx = off_by_one_element(to_t(rng.standard_normal((m, k)), dtype).to(DEV))
        x = tx.double().cpu().numpy()
        got = bf8.matmul(tx, gpu(w), gpu(s), bs)
        assert bf8.last_route() == 5
        check_bound(got.float().cpu().numpy(), x @ wd.T, np.abs(x) @ np.abs(wd).T, k, dtype, f"general M {m} N {n}")
    # K fits, the block width does not; exact integers, bit for bit
    w, s = exact_weights(40, 96), exact_scales(40, 96, (16, 24))
    x = rng.integers(-2, 3, (4, 96)).astype(np.float64)
    got = bf8.matmul(to_t(x, dtype).to(DEV), gpu(w), gpu(s), (16, 24))
    assert bf8.last_route() == 5 and np.array_equal(bits(got), bits(to_t(x @ dequant_f64(w, s, (16, 24)).T, dtype)))
    # a weight base that is not 16-byte aligned
    w, s = exact_weights(41, 128), exact_scales(40, 128, (16, 32))
    wt = gpu(w).reshape(-1)[120:120 + 40 * 128].reshape(40, 128)  # a [40, 128] view that starts 8 bytes before row 1
    assert wt.data_ptr() % 16 == 8 and wt.is_contiguous()
    x = rng.integers(-2, 3, (2, 128)).astype(np.float64)
    got = bf8.matmul(to_t(x, dtype).to(DEV), wt, gpu(s), (16, 32))
    assert bf8.last_route() == 5 and np.array_equal(bits(got), bits(to_t(x @ dequant_f64(wt.cpu().numpy(), s, (16, 32)).T, dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_gemv_rows_do_not_depend_on_m(dtype):
    """Route 1: fixed 2048-k staging chunks and 32 lanes per weight row, so row m of an M = 8 call has the bits of the M = 1 call on that row."""
    rng = np.random.default_rng(6)
    n, k, bs = 72, 2176, (128, 128)
    w, s = gpu(random_weights(rng, n, k)), gpu(random_scales(rng, (n, k), bs))
    tx = to_t(rng.standard_normal((8, k)), dtype).to(DEV)
    whole = bf8.matmul(tx, w, s, bs)
    assert bf8.last_route() == 1
    rows = torch.cat([bf8.matmul(tx[i:i + 1], w, s, bs) for i in range(8)], 0)
    assert np.array_equal(bits(whole), bits(rows))


# ------------------------------------------------------------------------------------------------ MoE
E, TOPK, MOE_N, MOE_K, SENTINEL = 4, 2, 136, 256, 7.0


def moe_indices(rng, t):
    idx = rng.integers(0, E - 1, (t, TOPK))  # expert 3 is never chosen
    idx[t // 2, TOPK - 1] = E + 1            # outside the expert range: its output row keeps the sentinel
    return idx


def moe_oracle(x3, wd, idx):
    """x3 [T, topk, K] f64 (already broadcast), wd [E, N, K] f64"""
    t = idx.shape[0]
    exact, mag = np.full((t, TOPK, MOE_N), np.nan), np.zeros((t, TOPK, MOE_N))
    for i in range(t):
        for sl in range(TOPK):
            e = int(idx[i, sl])
            if e < E:
                exact[i, sl], mag[i, sl] = wd[e] @ x3[i, sl], np.abs(wd[e]) @ np.abs(x3[i, sl])
    return exact, mag


def moe_layouts(tx3):
    """[T, topk, K] with equal slots -> the three input layouts of the same problem; else only the full one"""
    return {"T,K": tx3[:, 0], "T,1,K": tx3[:, :1], "T,topk,K": tx3}


@pytest.mark.parametrize("tokens", [1, 3, 5, 20])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("bs", BLOCKS, ids=str)
@pytest.mark.parametrize("exact_ints", [True, False], ids=["exact", "random"])
def test_moe(tokens, dtype, bs, exact_ints):
    rng = np.random.default_rng(tokens * 10 + exact_ints)
    if exact_ints:
        w = np.stack([exact_weights(MOE_N, MOE_K, e) for e in range(E)])
        s = np.stack([exact_scales(MOE_N, MOE_K, bs, 1, e) for e in range(E)])
    else:
        w, s = random_weights(rng, E, MOE_N, MOE_K), random_scales(rng, (E, MOE_N, MOE_K), bs, 1)
    wd = dequant_f64(w, s, bs)
    tw, ts = gpu(w), gpu(s)
    idx = moe_indices(rng, tokens)
    tidx = gpu(idx.astype(np.int32))
    want_route = 4 if tokens * TOPK > 8 else 3
    for shared in (True, False):  # every slot of a token reads the same row / its own row
        shape = (tokens, 1, MOE_K) if shared else (tokens, TOPK, MOE_K)
        tx3 = to_t(rng.integers(-2, 3, shape) if exact_ints else rng.standard_normal(shape), dtype).to(DEV).expand(tokens, TOPK, MOE_K)
        exact, mag = moe_oracle(tx3.double().cpu().numpy(), wd, idx)
        skipped = np.isnan(exact)
        assert skipped.sum() == MOE_N
        exact = np.where(skipped, SENTINEL, exact)
        for name, tx in (moe_layouts(tx3) if shared else {"T,topk,K": tx3}).items():
            out = torch.full((tokens, TOPK, MOE_N), SENTINEL, dtype=dtype, device=DEV)
            got = bf8.indexed_moe_gemm(tx, tw, ts, tidx, bs, out=out)
            assert bf8.last_route() == want_route, (tokens, bf8.last_route())
            what = f"moe T {tokens} blocks {bs} layout {name} shared {shared}"
            if exact_ints:
                assert np.array_equal(bits(got), bits(to_t(exact, dtype))), what
            else:
                g = got.float().cpu().numpy()
                assert np.all(g[skipped] == SENTINEL), what
                check_bound(g, exact, mag, MOE_K, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_moe_routes_3_and_4_agree_bit_for_bit(dtype):
    rng = np.random.default_rng(8)
    bs = (128, 128)
    w = gpu(np.stack([exact_weights(MOE_N, MOE_K, e) for e in range(E)]))
    s = gpu(np.stack([exact_scales(MOE_N, MOE_K, bs, 0, e) for e in range(E)]))
    tx = to_t(rng.integers(-2, 3, (20, TOPK, MOE_K)), dtype).to(DEV)
    idx = gpu(rng.integers(0, E, (20, TOPK)).astype(np.int32))
    grouped = bf8.indexed_moe_gemm(tx, w, s, idx, bs)
    assert bf8.last_route() == 4
    per_slot = torch.cat([bf8.indexed_moe_gemm(tx[i:i + 4], w, s, idx[i:i + 4], bs) for i in range(0, 20, 4)], 0)
    assert bf8.last_route() == 3
    assert np.array_equal(bits(grouped), bits(per_slot))


# ------------------------------------------------------------------------------------------------ the layer
def test_layer_forward_quantize_gather():
    rng = np.random.default_rng(9)
    n, k, bs, dt = 136, 256, (128, 128), torch.bfloat16
    w = torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32))
    bias = to_t(rng.uniform(-1, 1, n), dt).to(DEV)
    layer = bf8.BlockwiseFP8Linear.quantize(w.to(DEV), bs, bias, dequant_dtype=dt)
    want_q, want_s = quant_oracle(w.numpy(), *bs)
    assert np.array_equal(layer.weight.cpu().numpy(), want_q) and np.array_equal(layer.weight_scale_inv.cpu().numpy().view(np.int32), want_s.view(np.int32))
    assert np.array_equal(bits(layer.dequantize_w()), bits(torch.from_numpy(dequant_f32(want_q, want_s, bs)).to(dt)))  # the oracle's round trip
    assert layer.has_bias() and layer.name() == "blockwise-fp8-linear" and layer.dtype_and_device()[1] == layer.weight.device
    x = to_t(rng.standard_normal((2, 3, k)), dt).to(DEV)
    y = layer.forward(x)
    raw = bf8.matmul(x.reshape(6, k), layer.weight, layer.weight_scale_inv, bs)
    assert tuple(y.shape) == (2, 3, n) and y.dtype == dt and np.array_equal(bits(y), bits((raw + bias).reshape(2, 3, n)))
    with pytest.raises(ValueError, match="Weight shape mismatch"):
        layer.forward(x[..., :128])
    # stacked experts: gather_forward against dequantize_w (f32: one rounding of each weight, far inside the bound's slack) and a per-slot f64 matmul
    we, se = random_weights(rng, E, MOE_N, MOE_K), random_scales(rng, (E, MOE_N, MOE_K), bs)
    experts = bf8.BlockwiseFP8Linear(gpu(we), gpu(se), None, torch.float32, bs)
    wd = experts.dequantize_w().double().cpu().numpy()
    idx = rng.integers(0, E, (5, TOPK))
    tx = to_t(rng.standard_normal((5, MOE_K)), dt).to(DEV)
    got = experts.gather_forward(tx, gpu(idx.astype(np.int64)))
    x3 = np.repeat(tx.double().cpu().numpy()[:, None], TOPK, 1)
    exact, mag = moe_oracle(x3, wd, idx)
    assert tuple(got.shape) == (5, TOPK, MOE_N)
    check_bound(got.float().cpu().numpy(), exact, mag, MOE_K, dt, "layer.gather_forward")
    assert np.array_equal(bits(experts.gather_forward(tx[:, None, :], gpu(idx.astype(np.int32)))), bits(got))
    with pytest.raises(ValueError, match="Expected input to be rank 2 or 3"):
        experts.gather_forward(tx[0], gpu(idx.astype(np.int32)))


def test_layer_apply_isq():
    from mistralrs_amd import hqq, isq, mxfp4
    from mistralrs_amd.gguf.matmul import GgufMatMul
    from mistralrs_amd.gguf.qtensor import GgmlDType
    rng = np.random.default_rng(10)
    n, k, bs, dt = 128, 256, (128, 128), torch.bfloat16
    bias = to_t(rng.uniform(-1, 1, n), dt).to(DEV)
    layer = bf8.BlockwiseFP8Linear(gpu(random_weights(rng, n, k)), gpu(random_scales(rng, (n, k), bs)), bias, dt, bs)
    dense = layer.dequantize_w()
    x = to_t(rng.standard_normal((3, k)), dt).to(DEV)
    for target in (GgmlDType.Q8_0, GgmlDType.Q4K):
        got = layer.apply_isq(target)
        assert isinstance(got, GgufMatMul) and got.w.dtype == target and got.b.dtype == torch.float32
        want = GgufMatMul(isq.quantize(dense, target), bias.float())
        assert torch.equal(got.w.data, want.w.data) and np.array_equal(bits(got.forward(x)), bits(want.forward(x)))
    got = layer.apply_isq("MXFP4")
    assert isinstance(got, mxfp4.MXFP4Layer) and np.array_equal(bits(got.forward(x)), bits(mxfp4.MXFP4Layer.quantize(dense, bias).forward(x)))
    got = layer.apply_isq(None, imatrix_weight=[1.0] * k)  # the imatrix is ignored
    assert isinstance(got, bf8.UnquantLinear) and np.array_equal(bits(got.dequantize_w()), bits(dense))
    assert np.array_equal(bits(got.forward(x)), bits(torch.nn.functional.linear(x, dense, bias)))
    got = layer.apply_isq("HQQ8")
    assert isinstance(got, hqq.HqqLayer) and got.cfg.bits == 8 and got.cfg.group_size == 64 and got.bias is not None
    with pytest.raises(ValueError, match="HQQ does not support imatrix."):
        layer.apply_isq("HQQ4", imatrix_weight=[1.0] * k)
    with pytest.raises(ValueError, match="MXFP4 does not support imatrix."):
        layer.apply_isq("MXFP4", imatrix_weight=[1.0] * k)


def test_sharded_load():
    rng = np.random.default_rng(11)
    n, k, bs, dt = 256, 384, (128, 128), torch.bfloat16
    cfg = {"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": list(bs), "activation_scheme": "dynamic", "modules_to_not_convert": ["lm_head"]}
    w, s = random_weights(rng, n, k), random_scales(rng, (n, k), bs)
    tensors = {"l.weight": torch.from_numpy(w).view(torch.float8_e4m3fn), "l.weight_scale_inv": torch.from_numpy(s), "l.bias": to_t(rng.uniform(-1, 1, n), dt)}
    x = to_t(rng.standard_normal((3, k)), dt).to(DEV)
    whole = bf8.blockwise_fp8_linear_b(k, n, cfg, True, None, tensors, "l", dt, DEV)
    y = whole.forward(x)
    for rank in range(2):  # rows: the exact slice (the bias is the caller's to narrow, as in the reference's `vb.get((out_dim,), "bias")`)
        part = bf8.blockwise_fp8_linear_b(k, n, cfg, False, Shard(dim=0, rank=rank, world_size=2), tensors, "l", dt, DEV)
        assert tuple(part.weight.shape) == (128, k) and tuple(part.weight_scale_inv.shape) == (1, 3)
        assert np.array_equal(bits(part.forward(x) + whole.bias[rank * 128:(rank + 1) * 128]), bits(y[:, rank * 128:(rank + 1) * 128]))
    wd = dequant_f64(w, s, bs)
    xs = x.double().cpu().numpy()
    total, lim = np.zeros((3, n)), np.zeros((3, n))
    for rank in range(3):  # columns: partial sums, each under the bound of its own K range
        part = bf8.blockwise_fp8_linear_b(k, n, cfg, False, Shard(dim=1, rank=rank, world_size=3), tensors, "l", dt, DEV)
        assert tuple(part.weight.shape) == (n, 128) and tuple(part.weight_scale_inv.shape) == (2, 1)
        cols = slice(rank * 128, (rank + 1) * 128)
        got = part.forward(x[:, cols]).float().cpu().numpy()
        check_bound(got, xs[:, cols] @ wd[:, cols].T, np.abs(xs[:, cols]) @ np.abs(wd[:, cols]).T, 128, dt, f"column shard {rank}")
        total += got
        lim += 2.0 * (128 + 4) * 2.0 ** -24 * (np.abs(xs[:, cols]) @ np.abs(wd[:, cols]).T) * (1 + U[dt]) + U[dt] * np.abs(xs[:, cols] @ wd[:, cols].T)
    assert np.all(np.abs(total - xs @ wd.T) <= lim)  # the partial results add up to the unsharded product within the sum of their bounds
    with pytest.raises(ValueError, match="not aligned"):
        bf8.blockwise_fp8_linear_b(k, n, cfg, False, Shard(dim=1, rank=0, world_size=2), tensors, "l", dt, DEV)
