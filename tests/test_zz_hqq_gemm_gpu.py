"""GPU: the fused HQQ prompt GEMM (csrc/ext_hqq_gemm.hip, `HqqLayer.forward` above 8 rows) against numpy in f64 over oracle.hqq_oracle.dequantize.
The decode is compared bit for bit through x = I; sums that are exact in T (asserted on the CPU) bit for bit; random values element by element, no exclusions,
against the f32-accumulation bound of tests/test_bnb.py.  As built the tile is 128 columns (8 group rows x 16 n_lo) x 64 k, 64 rows up to M = 64 and 128 above,
and K splits over up to 8 workgroups of at least 8 k-steps while the grid stays under 256 workgroups: K = 960 is the largest that never splits, K = 976 the
smallest that does (here: in two), K = 2096 splits in four with a short last split; K = 80 and 976 end inside a k-step; N = 1088 has R = 17 (an n_lo edge)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mistralrs_amd  # noqa: F401
from mistralrs_amd import _lib, hqq
from oracle import hqq_oracle as H
from tests.test_bnb import check_bound, rne

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = [(4, "bfloat16"), (4, "float16"), (8, "bfloat16"), (8, "float16")]
TORCH = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}
SHAPES = [(9, 64, 64), (64, 1088, 80), (64, 64, 960), (65, 2048, 960), (9, 2048, 976), (128, 1088, 976), (129, 64, 976), (261, 1088, 976), (261, 2048, 80),
          (65, 1088, 2096)]  # (M, N, K)
GEMM_ARGS = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]


def layer_of(bits, dtype, q, scale, zero, n, k, bias=None):
    """(HqqLayer in `dtype` from unpacked codes q [64, w] and f32 scale / zero [w] / bias [n] holding T values, W_hat [n, k] in f64)"""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(TORCH[dtype])
    wq = H.pack(bits, q)
    layer = hqq.HqqLayer(torch.from_numpy(wq).to(DEV), t(zero), t(scale), (n, k), hqq.HqqConfig(bits=bits), t(bias))
    return layer, H.dequantize(bits, wq, scale, zero, {"bfloat16": "bf16", "float16": "f16", "float32": "f32"}[dtype]).reshape(n, k).astype(np.float64)


def random_layer(rng, bits, dtype, n, k, bias=False):
    w = n * k // 64
    scale = rne(rng.uniform(0.001, 0.05, w) * rng.choice([1.0, -1.0], w), dtype)[0]
    zero = rne(rng.uniform(0.0, 2 ** bits - 1.0, w), dtype)[0]
    b = rne(rng.uniform(-1, 1, n), dtype)[0] if bias else None
    return layer_of(bits, dtype, rng.integers(0, 2 ** bits, (64, w)).astype(np.uint8), scale, zero, n, k, b) + (b,)


@pytest.fixture
def every_m(monkeypatch):
    """`forward` sends rows above the measured crossover back to dequantize + matmul; the kernel itself is checked at every M"""
    monkeypatch.setattr(hqq, "MFMA_MAX_ROWS", 1 << 30)


def bits_of(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def test_route():
    rng = np.random.default_rng(1)
    layer, _, _ = random_layer(rng, 4, "bfloat16", 128, 64)
    x = torch.randn(9, 64, device=DEV, dtype=torch.bfloat16)
    y = layer.forward(x)
    assert hqq.last_route() == "mfma" and y.dtype == torch.bfloat16 and tuple(y.shape) == (9, 128)
    out = torch.empty_like(y)
    rc = _lib.sym("ext", "mrs_hqq_gemm", GEMM_ARGS, C.c_int)(4, 2, layer.w_q.data_ptr(), layer.scales.data_ptr(), layer.zeros.data_ptr(), None, x.data_ptr(), 64,
                                                            out.data_ptr(), 128, 128, 64, 9, None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(out.view(torch.int16), y.view(torch.int16))
    layer.forward(x[:8])
    assert hqq.last_route() == "gemv"
    layer.forward(torch.randn(hqq.MFMA_MAX_ROWS + 1, 64, device=DEV, dtype=torch.bfloat16))
    assert hqq.last_route() == "dense"  # above the measured crossover
    random_layer(rng, 4, "float32", 128, 64)[0].forward(x.float())
    assert hqq.last_route() == "dense"


@pytest.mark.parametrize("n,k", [(64, 16), (1088, 80)])
@pytest.mark.parametrize("bits,dtype", KINDS)
def test_decode_bit_for_bit(bits, dtype, n, k):
    rng = np.random.default_rng(2)
    w = n * k // 64
    q = rng.permutation(np.arange(64 * w) % 2 ** bits).reshape(64, w).astype(np.uint8)
    assert all(len(np.unique(part)) == 2 ** bits for part in ((q[:32], q[32:]) if bits == 4 else (q,)))  # every code value in every nibble position
    scale = rne(rng.uniform(0.001, 0.05, w) * rng.choice([1.0, -1.0], w), dtype)[0]
    layer, W = layer_of(bits, dtype, q, scale, rne(rng.uniform(0.0, 2 ** bits - 1.0, w), dtype)[0], n, k)
    got = layer.forward(torch.eye(k, device=DEV, dtype=TORCH[dtype]))
    assert hqq.last_route() == "mfma"
    assert np.array_equal(got.float().cpu().numpy().astype(np.float64), W.T)


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("bits,dtype", KINDS)
def test_exact_sums_bit_for_bit(every_m, bits, dtype, m, n, k):
    """At most 35 non-zero x per row (one in every k-step, the first and the last column), |W_hat| in {0, 1/2, 1, 2}, |bias| <= 3: |sum| <= 73 on a grid of 1/2."""
    rng = np.random.default_rng(3)
    w = n * k // 64
    zero = rng.integers(1, 2 ** bits - 1, w).astype(np.float64)
    q = (zero[None, :] + rng.integers(-1, 2, (64, w))).astype(np.uint8)
    scale = 2.0 ** rng.integers(-1, 2, w) * rng.choice([1.0, -1.0], w)
    bias = rng.integers(-3, 4, n).astype(np.float64)
    layer, W = layer_of(bits, dtype, q, scale, zero, n, k, bias)
    cols = np.unique(np.concatenate([[0, k - 1], [rng.integers(s, min(k, s + 64)) for s in range(0, k, 64)]]))
    x = np.zeros((m, k))
    x[:, cols] = rng.integers(-1, 2, (m, len(cols)))
    E = x @ W.T + bias
    assert np.array_equal(rne(E, dtype)[0].astype(np.float64), E)  # CPU: E is a T value, so every summation order gives it
    got = layer.forward(torch.from_numpy(x).to(DEV).to(TORCH[dtype]))
    assert hqq.last_route() == "mfma"
    assert np.array_equal(bits_of(got), rne(E, dtype)[1].reshape(m, n))


@pytest.mark.parametrize("shape,n,k,xdtype", [((m,), n, k, None) for m, n, k in SHAPES] + [((2, 5), 1088, 80, None), ((33,), 64, 976, "float32")])
@pytest.mark.parametrize("bits,dtype", KINDS)
def test_random_values_inside_the_bound(every_m, bits, dtype, shape, n, k, xdtype):
    rng = np.random.default_rng(4)
    m = int(np.prod(shape))
    for with_bias in (False, True):
        layer, W, bias = random_layer(rng, bits, dtype, n, k, with_bias)
        x32 = rng.standard_normal((m, k)).astype(np.float32)
        x = rne(x32, dtype)[0].astype(np.float64)  # what the layer's cast gives
        src = torch.from_numpy(x32 if xdtype else rne(x32, dtype)[0]).to(DEV).to(TORCH[xdtype or dtype])
        got = layer.forward(src.reshape(*shape, k))
        assert hqq.last_route() == "mfma" and got.dtype == TORCH[dtype] and tuple(got.shape) == (*shape, n)
        E = x @ W.T + (0.0 if bias is None else bias)
        mag = np.abs(x) @ np.abs(W.T) + (0.0 if bias is None else np.abs(bias))
        check_bound(got.float().cpu().numpy().reshape(m, n), E, mag, k, dtype, f"hqq{bits} {dtype} {shape} N {n} K {k} bias {with_bias}")


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("bits", [4, 8])
def test_nothing_outside_the_output_is_written(every_m, bits, m, n, k):
    layer, _, _ = random_layer(np.random.default_rng(5), bits, "bfloat16", n, k, True)
    x = torch.randn(m, k, device=DEV, dtype=torch.bfloat16)
    want = layer.forward(x)
    ldo = n + 24
    out = torch.full((m + 3, ldo), -777.0, dtype=torch.bfloat16, device=DEV)
    floats = _lib.sym("ext", "mrs_hqq_gemm_workspace_floats", [C.c_int] * 3, C.c_size_t)(n, k, m)
    ws = torch.full((floats + 64,), -777.0, dtype=torch.float32, device=DEV)
    rc = _lib.sym("ext", "mrs_hqq_gemm", GEMM_ARGS, C.c_int)(bits, 2, layer.w_q.data_ptr(), layer.scales.data_ptr(), layer.zeros.data_ptr(), layer.bias.data_ptr(),
                                                            x.data_ptr(), k, out.data_ptr(), ldo, n, k, m, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(out[:m, :n].contiguous().view(torch.int16), want.view(torch.int16))
    assert bool((out[m:] == -777.0).all()) and bool((out[:, n:] == -777.0).all()) and bool((ws[floats:] == -777.0).all())
