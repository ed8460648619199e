"""GPU: the bitsandbytes kernels (dequantize; matmul on routes 1 / 2 / 3), the reference's nine C symbols and `BnbLinear` against the numpy oracle of
tests/test_bnb.py.  Dequantize and the exact matmul cases (dyadic table values, power-of-two absmax, small integer x and bias: the result is exact in T, asserted
on the CPU, so any summation order must give it) are compared bit for bit; random matmul cases are held element by element, with no exclusions, to the bound
stated in tests/test_bnb.py.  Route 1 as built stages activations in chunks of 2048 k (1024 for f32) and splits K over up to 8 workgroups of at least 1024 k
each, so its K list holds 1984 / 2048 / 2112 (one split | two; f32: a second chunk) and 16384 / 16448 (a second chunk for 16-bit)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mistralrs_amd  # noqa: F401
from mistralrs_amd import _lib, bnb
from tests.test_bnb import T_MAX, TABLES, absmax_f32, check_bound, checkpoint, dequantize, pack_nibbles, rne

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SENTINEL = -777.0
EXACT_CODES = {"nf4": [0, 7, 15], "fp4": [0, 8, 3, 11, 5, 13, 7, 15]}  # -1, 0, 1 | +-0, +-1, +-0.5, +-0.25


def gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(DTYPES[dtype])


def bits_of(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def nested_of(rng, blocks, nbs=256, exact=False):
    """(u8 absmax, (nested_absmax, nested_quant_map, nested_blocksize, nested_offset)); `exact`: every A_b is 0.5, 1 or 2"""
    nqm = np.sort(rng.uniform(-1, 1, 256)).astype(np.float32)
    if exact:
        nqm[:3] = [0.25, 0.75, 1.75]
        return rng.integers(0, 3, blocks).astype(np.uint8), (np.ones(-(-blocks // nbs), np.float32), nqm, nbs, 0.25)
    return rng.integers(0, 256, blocks).astype(np.uint8), (rng.uniform(0.005, 0.02, -(-blocks // nbs)).astype(np.float32), nqm, nbs, 0.02)


def nested_kw(nested):
    return {} if nested is None else dict(nested_absmax=gpu(nested[0]), nested_quant_map=gpu(nested[1]), nested_blocksize=nested[2], nested_offset=nested[3])


# ------------------------------------------------------------------------------------------------ dequantize
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("qt", ["nf4", "fp4", "int8"])
def test_dequantize_bit_exact(qt, dtype):
    rng = np.random.default_rng(11)
    ncodes = 256 if qt == "int8" else 16
    code = np.sort(rng.uniform(-1, 1, 256)).astype(np.float32) if qt == "int8" else TABLES[qt]
    tiny = 2.0 ** -130 if dtype == "bfloat16" else 2.0 ** -20  # makes every f16 / bf16 result subnormal
    fn = getattr(_lib.load("quant"), f"dequantize_blockwise_{ {'float32': 'f32', 'float16': 'f16', 'bfloat16': 'bf16'}[dtype]}_{qt}")
    fn.argtypes, fn.restype = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p], None
    cases = [(bs, n, None) for bs in (64, 256, 4096) for n in (bs, 3 * bs, 2 * bs + 37)] + ([(64, 300 * 64, 256)] if qt != "int8" else [])
    for bs, n, nbs in cases:
        codes = rng.permutation(np.arange(n) % ncodes).astype(np.uint8)
        assert len(np.unique(codes)) == min(n, ncodes)  # every code value is present
        blocks = -(-n // bs)
        absmax = rng.uniform(0.01, 2.0, blocks).astype(np.float32)
        absmax[0], absmax[-1] = tiny, T_MAX[dtype]  # one block: the largest finite absmax
        nested = None
        if nbs:
            absmax, nested = nested_of(rng, blocks, nbs)
            assert len(nested[0]) == 2 and blocks % nbs  # a second, partial nested block
        want = dequantize(codes, code, absmax, bs, dtype, nested)[1]
        packed = gpu(codes if qt == "int8" else pack_nibbles(codes))
        out = torch.full((n + 64,), SENTINEL, dtype=DTYPES[dtype], device=DEV)
        bnb.dequantize(packed, gpu(absmax), qt, bs, n, DTYPES[dtype], code=gpu(code) if qt == "int8" else None, out=out, **nested_kw(nested))
        what = (qt, dtype, bs, n, nbs)
        assert np.array_equal(bits_of(out[:n]), want) and bool((out[n:] == SENTINEL).all()), what
        if nested is None:  # the reference's symbol: plain absmax only
            out.fill_(SENTINEL)
            torch.cuda.synchronize()
            tc, ta = gpu(code), gpu(absmax)  # named: alive over the call
            fn(tc.data_ptr(), packed.data_ptr(), ta.data_ptr(), out.data_ptr(), bs, n, None)
            torch.cuda.synchronize()
            assert np.array_equal(bits_of(out[:n]), want) and bool((out[n:] == SENTINEL).all()), what
        if qt != "int8":
            w = bnb.BnbLinear.from_parts(packed, gpu(absmax), qt, bs, (1, n), DTYPES[dtype], **nested_kw(nested)).dequantize_w()
            assert tuple(w.shape) == (1, n) and np.array_equal(bits_of(w).reshape(-1), want), what


# ------------------------------------------------------------------------------------------------ matmul
def route_cases(dtype):
    """(route, blocksize, Ms, N, K)"""
    out = [(1, bs, (1, 2, 7, 8), n, k) for n in (1, 9, 33) for bs, ks in ((64, (64, 192, 1984, 2048, 2112, 16384, 16448)), (4096, (4096, 3 * 4096))) for k in ks]
    if dtype != "float32":
        out += [(2, 64, (9, 33, 65, 129), n, k) for n in (32, 96, 160) for k in (64, 192, 320)] + [(2, 4096, (33,), 96, 4096)]
    else:
        out.append((3, 64, (9,), 32, 64))
    return out + [(3, 64, (3,), 5, 96)]  # 7.5 blocks: blocks straddle rows, the last one is partial


def run_matmul(rng, dtype, exact):
    case = 0
    for route, bs, ms, n, k in route_cases(dtype):
        for with_nested in (False, True):
            qt = ("nf4", "fp4")[case % 2]
            case += 1
            blocks = -(-n * k // bs)
            if exact:
                codes = rng.choice(EXACT_CODES[qt], n * k).astype(np.uint8)
                absmax, nested = nested_of(rng, blocks, exact=True) if with_nested else ((2.0 ** rng.integers(-1, 2, blocks)).astype(np.float32), None)
            else:
                codes = rng.integers(0, 16, n * k).astype(np.uint8)
                absmax, nested = nested_of(rng, blocks) if with_nested else (rng.uniform(0.005, 0.02, blocks).astype(np.float32), None)
            w = dequantize(codes, TABLES[qt], absmax, bs, dtype, nested)[0].reshape(n, k).astype(np.float64)
            tw, ta, kw = gpu(pack_nibbles(codes)), gpu(absmax), nested_kw(nested)
            for m in ms:
                if exact:  # at most six non-zero x per row, |x| <= 2, |W_hat| <= 2 on a grid of 1/8, |bias| <= 3: |sum| <= 27 on that grid is exact in bf16
                    x = np.zeros((m, k))
                    cols = np.concatenate([[0, k - 1], rng.integers(0, k, 4)])
                    x[:, cols] = rng.integers(-2, 3, (m, 6))
                    biases = (None, rng.integers(-3, 4, n).astype(np.float64))
                else:
                    x = rne(rng.standard_normal((m, k)), dtype)[0].astype(np.float64)
                    biases = (None, rne(rng.uniform(-1, 1, n), dtype)[0].astype(np.float64))
                tx = gpu_t(x, dtype)
                for bias in biases:
                    E = x @ w.T + (0.0 if bias is None else bias)
                    what = f"{qt} {dtype} route {route} bs {bs} M {m} N {n} K {k} nested {with_nested} bias {bias is not None}"
                    out = torch.full((m, n), SENTINEL, dtype=DTYPES[dtype], device=DEV)
                    got = bnb.matmul(tx, tw, ta, qt, bs, n, gpu_t(bias, dtype), out=out, **kw)
                    assert bnb.last_route() == route, what
                    if exact:
                        assert np.array_equal(rne(E, dtype)[0].astype(np.float64), E), what  # CPU: E is a T value
                        assert np.array_equal(bits_of(got), rne(E, dtype)[1].reshape(m, n)), what
                    else:
                        check_bound(got.float().cpu().numpy(), E, np.abs(x) @ np.abs(w.T) + (0.0 if bias is None else np.abs(bias)), k, dtype, what)
                    if route == 1 and m == 8:  # a row of an M = 8 call has the bits of its own M = 1 call
                        one = bnb.matmul(tx[5:6], tw, ta, qt, bs, n, gpu_t(bias, dtype), **kw)
                        assert np.array_equal(bits_of(one), bits_of(got[5:6])), what


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_matmul_exact_cases_bit_for_bit(dtype):
    run_matmul(np.random.default_rng(21), dtype, exact=True)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_matmul_random_cases_inside_the_bound(dtype):
    run_matmul(np.random.default_rng(22), dtype, exact=False)


# ------------------------------------------------------------------------------------------------ layer and loader
@pytest.mark.parametrize("qt,nested", [("nf4", True), ("fp4", False)])
def test_layer_and_loader(qt, nested):
    rng = np.random.default_rng(31)
    n, k, bs = 33, 192, 64
    t, state = checkpoint(rng, qt, n, k, bs, nested)
    t["m.bias"] = torch.from_numpy(rng.uniform(-1, 1, n).astype(np.float32)).to(torch.bfloat16)
    layer = bnb.bnb_linear_b(k, n, True, t, "m", device=DEV)
    codes = np.stack([t["m.weight"].numpy().reshape(-1) >> 4, t["m.weight"].numpy().reshape(-1) & 15], 1).reshape(-1)
    nest = (t["m.weight.nested_absmax"].numpy(), t["m.weight.nested_quant_map"].numpy(), 256, state["nested_offset"]) if nested else None
    w32, wbits = dequantize(codes, TABLES[qt], t["m.weight.absmax"].numpy(), bs, "bfloat16", nest)
    assert absmax_f32(t["m.weight.absmax"].numpy(), nest).dtype == np.float32
    dense = layer.dequantize_w()
    assert dense.dtype == torch.bfloat16 and np.array_equal(bits_of(dense).reshape(-1), wbits)
    plain = layer.apply_isq(None)
    assert plain.name() == "unquant-linear" and plain.has_bias() and torch.equal(plain.dequantize_w(), dense)
    x = torch.from_numpy(rng.standard_normal((2, 3, k)).astype(np.float32)).to(DEV)
    y = layer.forward(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == (2, 3, n) and bnb.last_route() == 1
    xb = x.to(torch.bfloat16).float().cpu().numpy().reshape(6, k).astype(np.float64)
    bias = t["m.bias"].float().numpy().astype(np.float64)
    w = w32.reshape(n, k).astype(np.float64)
    check_bound(y.cpu().numpy().reshape(6, n), xb @ w.T + bias, np.abs(xb) @ np.abs(w.T) + np.abs(bias), k, "bfloat16", f"layer {qt}")
