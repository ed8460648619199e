"""GPU: the MXFP4 kernels (dequantize, dense matmul on every route, MoE gather) and `MXFP4Layer` against a numpy oracle written from the format definition:
weights dequantized exactly, f64 sums.  Exact-integer cases are compared bit for bit; random cases are held, element by element and with no exclusions, to

    |out - exact| <= B (1 + u_T) + u_T |exact|,   B = 2 K 2^-24 (sum |x w| + |bias|),   u_T = 2^-8 (bf16) / 2^-11 (f16)

(K 2^-24 sum |x w| bounds any order of round-to-nearest f32 additions of the exact products; the factor 2 covers a truncating adder in the matrix core).
u_T |exact| models one rounding in the normal range of T.  With scale bytes 107..137 some f16 results leave that range, and there the format decides: a sum
past 65520 must come out as the infinity of its sign, and a sum below 2^-14 sits on the fixed 2^-24 grid, where one rounding is off by up to 2^-25."""
import numpy as np
import pytest
import torch

import mistralrs_amd  # noqa: F401
from mistralrs_amd import mxfp4, uqff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP4 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.bfloat16, torch.float16]


# ------------------------------------------------------------------------------------------------ oracle
def nibbles(blocks: np.ndarray) -> np.ndarray:
    return np.stack([blocks & 15, blocks >> 4], -1).reshape(*blocks.shape[:-1], blocks.shape[-1] * 2)


def scale_f32(scales: np.ndarray) -> np.ndarray:
    return (scales.astype(np.uint32) << 23).view(np.float32)  # s = 0 -> 0.0


def dequant_f32(blocks, scales):
    with np.errstate(over="ignore"):  # 3 .. 6 x 2^127 is the f32 infinity, on the device too
        return FP4.astype(np.float32)[nibbles(blocks)] * np.repeat(scale_f32(scales), 32, -1)


def dequant_f64(blocks, scales):
    return FP4[nibbles(blocks)] * np.repeat(scale_f32(scales).astype(np.float64), 32, -1)


def asymmetric_weights(n, k, e=0):
    nn, kk = np.arange(n)[:, None], np.arange(k)[None, :]
    nib = (3 * nn + 5 * kk + (nn * kk) // 7 + 11 * e) % 16
    blocks = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    scales = (127 + (nn * 3 + np.arange(k // 32)[None, :] + e) % 2).astype(np.uint8)
    return blocks, scales


def random_weights(rng, *lead, k):
    return rng.integers(0, 256, (*lead, k // 2), dtype=np.uint8), rng.integers(107, 138, (*lead, k // 32)).astype(np.uint8)


def to_t(a, dtype):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype)


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


F16_OVERFLOW = 65520.0  # round-to-nearest-even gives inf from here on (halfway between 65504 and 2^16)


def check_bound(got, exact, mag, k, dtype, what):
    u = U[dtype]
    b = 2.0 * k * 2.0 ** -24 * mag
    got = got.astype(np.float64)
    lim = b * (1 + u) + u * np.abs(exact)
    if dtype == torch.float16:  # below 2^-14 f16 is a fixed grid of 2^-24: the one rounding there is off by up to 2^-25, which u_T |exact| does not model
        lim = lim + np.where(np.abs(exact) < 2.0 ** -14 + b, 2.0 ** -25, 0.0)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - exact) <= lim
    if dtype == torch.float16:  # scales up to 2^10 take some sums past the f16 range: there the one correct rounding is the infinity of the sum's sign
        inf_ok = np.isinf(got) & (np.sign(got) == np.sign(exact))
        must, may = np.abs(exact) - b >= F16_OVERFLOW, np.abs(exact) + b >= F16_OVERFLOW
        ok = np.where(must, inf_ok, np.where(may, ok | inf_ok, ok))
    fin = np.isfinite(got)
    worst = float(np.max(np.abs(got - exact)[fin] / np.maximum(lim[fin], 1e-300))) if fin.any() else 0.0
    print(f"{what}: worst error / bound = {worst:.3f}")
    bad = np.argwhere(~ok)
    assert not len(bad), (f"{what}: {len(bad)} of {ok.size} elements outside the bound (worst finite {worst:.2f}x); first at {tuple(bad[0])}: "
                          f"got {got[tuple(bad[0])]!r} exact {exact[tuple(bad[0])]!r} bound {lim[tuple(bad[0])]!r}")


# ------------------------------------------------------------------------------------------------ dequantize
def test_dequantize_rows():
    rng = np.random.default_rng(0)
    blocks = rng.integers(0, 256, (5, 48), dtype=np.uint8)
    scales = np.array([[0, 1, 127], [254, 120, 0], [1, 254, 130], [127, 127, 127], [113, 137, 1]], np.uint8)
    tb, ts = torch.from_numpy(blocks).to(DEV), torch.from_numpy(scales).to(DEV)
    got = mxfp4.dequantize_rows(tb, ts, None, torch.float32).cpu().numpy()
    assert np.array_equal(got.view(np.int32), dequant_f32(blocks, scales).view(np.int32))  # subnormals, signed zeros and s = 0 included
    scales2 = rng.integers(113, 138, (5, 3)).astype(np.uint8)
    ts2 = torch.from_numpy(scales2).to(DEV)
    want = torch.from_numpy(dequant_f32(blocks, scales2))
    for dt in DTYPES:
        assert np.array_equal(bits(mxfp4.dequantize_rows(tb, ts2, None, dt)), bits(want.to(dt)))
        ids = torch.tensor([4, 0, 4, 2], device=DEV)
        assert np.array_equal(bits(mxfp4.dequantize_rows(tb, ts2, ids, dt)), bits(want[[4, 0, 4, 2]].to(dt)))
    ids = torch.tensor([4, 0, 4, 2], device=DEV)
    assert np.array_equal(mxfp4.dequantize_rows(tb, ts, ids, torch.float32).cpu().numpy().view(np.int32), dequant_f32(blocks, scales)[[4, 0, 4, 2]].view(np.int32))


# ------------------------------------------------------------------------------------------------ dense
EXACT_SHAPES = [(1, 40), (3, 72), (8, 72), (9, 72), (33, 40), (70, 136)]


@pytest.mark.parametrize("k", [32, 96])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_dense_exact_integer(k, dtype):
    rng = np.random.default_rng(k)
    for m, n in EXACT_SHAPES:
        blocks, scales = asymmetric_weights(n, k)
        x = rng.integers(-2, 3, (m, k)).astype(np.float64)
        bias = rng.integers(-3, 4, n).astype(np.float64)
        w = dequant_f64(blocks, scales)
        tb, ts, tx = torch.from_numpy(blocks).to(DEV), torch.from_numpy(scales).to(DEV), to_t(x, dtype).to(DEV)
        for with_bias in (False, True):
            exact = x @ w.T + (bias if with_bias else 0.0)
            got = mxfp4.matmul(tx, tb, ts, to_t(bias, dtype).to(DEV) if with_bias else None)
            route = mxfp4.last_route()
            assert route == (1 if m <= 8 else 2 if dtype == torch.bfloat16 else 5), (m, route)
            assert np.array_equal(bits(got), bits(to_t(exact, dtype))), f"M {m} N {n} K {k} bias {with_bias}: differs from the correctly rounded exact result"


@pytest.mark.parametrize("k", [96, 2880])
@pytest.mark.parametrize("n", [72, 136])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_dense_random(k, n, dtype):
    rng = np.random.default_rng(1000 + k + n)
    blocks, scales = random_weights(rng, n, k=k)
    w = dequant_f64(blocks, scales)
    tb, ts = torch.from_numpy(blocks).to(DEV), torch.from_numpy(scales).to(DEV)
    tbias = to_t(rng.uniform(-2, 2, n), dtype)
    bias = tbias.double().numpy()
    for m in (1, 4, 5, 8, 9, 70):
        tx = to_t(rng.uniform(-2, 2, (m, k)), dtype)
        x = tx.double().numpy()
        for with_bias in (False, True):
            exact = x @ w.T + (bias if with_bias else 0.0)
            mag = np.abs(x) @ np.abs(w).T + (np.abs(bias) if with_bias else 0.0)
            got = mxfp4.matmul(tx.to(DEV), tb, ts, tbias.to(DEV) if with_bias else None).float().cpu().numpy()
            check_bound(got, exact, mag, k, dtype, f"dense M {m} N {n} K {k} bias {with_bias}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_route_identity_m8_equals_row_by_row(dtype):
    """The GEMV's per-row summation order does not depend on M (fixed 2048-k staging chunks, 32 lanes per weight row): one M = 8 call == eight M = 1 calls."""
    rng = np.random.default_rng(7)
    k, n = 2880, 72
    blocks, scales = random_weights(rng, n, k=k)
    tb, ts = torch.from_numpy(blocks).to(DEV), torch.from_numpy(scales).to(DEV)
    tx = to_t(rng.uniform(-2, 2, (8, k)), dtype).to(DEV)
    tbias = to_t(rng.uniform(-2, 2, n), dtype).to(DEV)
    whole = mxfp4.matmul(tx, tb, ts, tbias)
    rows = torch.cat([mxfp4.matmul(tx[i:i + 1], tb, ts, tbias) for i in range(8)], 0)
    assert np.array_equal(bits(whole), bits(rows))


# ------------------------------------------------------------------------------------------------ MoE
E, TOPK, MOE_N, MOE_K, SENTINEL = 4, 2, 72, 96, 7.0


def moe_oracle(x, w, bias, idx, has_topk):
    t = idx.shape[0]
    exact = np.full((t, TOPK, MOE_N), np.nan)
    mag = np.zeros((t, TOPK, MOE_N))
    for i in range(t):
        for s in range(TOPK):
            e = int(idx[i, s])
            if e >= E:
                continue
            row = x[i, s] if has_topk else x[i]
            exact[i, s] = w[e] @ row + (bias[e] if bias is not None else 0.0)
            mag[i, s] = np.abs(w[e]) @ np.abs(row) + (np.abs(bias[e]) if bias is not None else 0.0)
    return exact, mag


def index_patterns(rng, t):
    rand = rng.integers(0, E, (t, TOPK))
    one_expert = np.full((t, TOPK), 2)
    dropped = rng.integers(0, E, (t, TOPK))
    dropped[t // 2, TOPK - 1] = E  # outside the expert range: its output row keeps the sentinel
    return {"random": rand, "all_to_expert_2": one_expert, "one_slot_dropped": dropped}


@pytest.mark.parametrize("tokens", [1, 3, 17])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("exact_ints", [True, False], ids=["exact", "random"])
def test_moe(tokens, dtype, exact_ints):
    rng = np.random.default_rng(tokens * 10 + exact_ints)
    if exact_ints:
        bs = [asymmetric_weights(MOE_N, MOE_K, e) for e in range(E)]
        blocks, scales = np.stack([b for b, _ in bs]), np.stack([s for _, s in bs])
        tbias = to_t(rng.integers(-3, 4, (E, MOE_N)), dtype)
    else:
        blocks, scales = random_weights(rng, E, MOE_N, k=MOE_K)
        tbias = to_t(rng.uniform(-2, 2, (E, MOE_N)), dtype)
    w = dequant_f64(blocks, scales)
    tb, ts = torch.from_numpy(blocks).to(DEV), torch.from_numpy(scales).to(DEV)
    want_route = 4 if tokens * TOPK > 8 else 3
    for has_topk in (False, True):
        shape = (tokens, TOPK, MOE_K) if has_topk else (tokens, MOE_K)
        tx = to_t(rng.integers(-2, 3, shape) if exact_ints else rng.uniform(-2, 2, shape), dtype)
        x = tx.double().numpy()
        for name, idx in index_patterns(rng, tokens).items():
            tidx = torch.from_numpy(idx.astype(np.int32)).to(DEV)
            for with_bias in (False, True):
                exact, mag = moe_oracle(x, w, tbias.double().numpy() if with_bias else None, idx, has_topk)
                skipped = np.isnan(exact)
                assert skipped.any() == (name == "one_slot_dropped")
                exact = np.where(skipped, SENTINEL, exact)
                for entry in ("indexed", "grouped"):
                    out = torch.full((tokens, TOPK, MOE_N), SENTINEL, dtype=dtype, device=DEV)
                    got = mxfp4.indexed_moe_gemm(tx.to(DEV), tb, ts, tbias.to(DEV) if with_bias else None, tidx, out=out, entry=entry)
                    assert mxfp4.last_route() == want_route, (tokens, entry, mxfp4.last_route())
                    what = f"moe T {tokens} {name} topk_dim {has_topk} bias {with_bias} {entry}"
                    if exact_ints:
                        assert np.array_equal(bits(got), bits(to_t(exact, dtype))), what
                    else:
                        g = got.float().cpu().numpy()
                        assert np.all(g[skipped] == SENTINEL), what
                        check_bound(g, exact, mag, MOE_K, dtype, what)


# ------------------------------------------------------------------------------------------------ the layer
def test_layer_end_to_end(tmp_path):
    rng = np.random.default_rng(3)
    w = torch.from_numpy(rng.standard_normal((72, 96)).astype(np.float32)).to(DEV)
    bias = to_t(rng.uniform(-1, 1, 72), torch.bfloat16).to(DEV)
    layer = mxfp4.MXFP4Layer.quantize(w, bias)
    cb, cs = mxfp4.quantize_tensors(w.cpu())
    assert torch.equal(layer.blocks.cpu(), cb) and torch.equal(layer.scales.cpu(), cs)  # the quantizer gives the same bytes on either device
    x = to_t(rng.uniform(-2, 2, (2, 3, 96)), torch.bfloat16).to(DEV)
    y = layer.forward(x)
    assert tuple(y.shape) == (2, 3, 72) and y.dtype == torch.bfloat16
    wd = dequant_f64(layer.blocks.cpu().numpy(), layer.scales.cpu().numpy())
    xd = x.double().cpu().numpy().reshape(6, 96)
    check_bound(y.float().cpu().numpy().reshape(6, 72), xd @ wd.T + bias.double().cpu().numpy(), np.abs(xd) @ np.abs(wd).T + np.abs(bias.double().cpu().numpy()),
                96, torch.bfloat16, "layer.forward")
    assert np.array_equal(bits(layer.dequantize_w()), bits(torch.from_numpy(wd).float().to(torch.bfloat16)))
    ids = torch.tensor([[5, 0], [71, 5]], device=DEV)
    emb = layer.embedding_forward(ids)
    assert tuple(emb.shape) == (2, 2, 96) and np.array_equal(bits(emb), bits(layer.dequantize_w()[ids.reshape(-1)].reshape(2, 2, 96)))
    # UQFF round trip: identical forward bits
    path = str(tmp_path / "l.uqff")
    uqff.write(path, layer.serialize_uqff("l"))
    back = mxfp4.MXFP4Layer.from_uqff(uqff.UqffReader(path), "l", DEV)
    assert back.has_bias() and np.array_equal(bits(back.forward(x)), bits(y))
    # stacked experts: gather_forward == the raw launch; GPT-OSS [E, N, K/32, 16] blocks == the flat layout
    blocks, scales = random_weights(rng, 2, 8, k=96)
    b4 = torch.from_numpy(blocks.reshape(2, 8, 3, 16)).to(DEV)
    ts = torch.from_numpy(scales).to(DEV)
    experts = mxfp4.MXFP4Layer.from_parts(mxfp4.packed_gptoss_blocks(b4), ts, to_t(rng.uniform(-1, 1, (2, 8)), torch.bfloat16).to(DEV))
    assert np.array_equal(bits(experts.dequantize_w()), bits(torch.from_numpy(dequant_f32(blocks, scales)).to(torch.bfloat16)))
    xs = to_t(rng.uniform(-2, 2, (5, 96)), torch.bfloat16).to(DEV)
    idx = torch.from_numpy(rng.integers(0, 2, (5, 2)).astype(np.int32)).to(DEV)
    got = experts.gather_forward(xs, idx)
    raw = mxfp4.indexed_moe_gemm(xs, experts.blocks, experts.scales, experts.bias, idx, entry="grouped")
    assert tuple(got.shape) == (5, 2, 8) and np.array_equal(bits(got), bits(raw))
    got3 = experts.gather_forward(xs[:, None, :].expand(5, 2, 96), idx)
    assert np.array_equal(bits(got3), bits(got))
    with pytest.raises(ValueError, match="Expected input to be rank 2 or 3"):
        experts.gather_forward(xs[0], idx)
    with pytest.raises(ValueError, match="Weight shape mismatch"):
        layer.forward(x[..., :64])


def test_max_smem_optin_is_the_device_attribute():
    import ctypes
    torch.cuda.init()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)  # the HIP runtime this process already runs on
    hip = ctypes.CDLL(path)
    v = ctypes.c_int(0)
    rc = hip.hipDeviceGetAttribute(ctypes.byref(v), 75, 0)      # hipDeviceAttributeSharedMemPerBlockOptin
    if rc != 0 or v.value <= 0:
        assert hip.hipDeviceGetAttribute(ctypes.byref(v), 74, 0) == 0  # hipDeviceAttributeMaxSharedMemoryPerBlock
    assert v.value >= 64 * 1024
    assert mxfp4.max_smem_optin() == v.value
