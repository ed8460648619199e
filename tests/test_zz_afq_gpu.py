"""GPU: the AFQ kernels (dequantize, embedding, quantize, dense matmul on routes 1 / 2 / 5, MoE gather on routes 3 / 4), the reference's C symbols and `AfqLayer`
against the numpy oracle of tests/test_afq.py.  Dequantize, embedding and quantize are compared bit for bit, and so are the exact-integer matmul cases (every
intermediate value is an exact f32, so the result must be RNE_T(exact)).  Random cases are held, element by element and with no exclusions, to

    |out - E| <= B (1 + u_T) + u_T |E|,   B = 2 n_ops 2^-24 (sum |x_k| (q_k |s_g| + |b_g|) + |bias|),   n_ops = K + 4 K / group + 4  (2 K + ... for f32 x)

with E the f64 value of sum x_k (q_k s_g + b_g) + bias at the stored T values of s and b, and u_T = 2^-8 (bf16) / 2^-11 (f16) / 2^-24 (f32).  n_ops 2^-24 bounds
every f32 rounding on the way of a term (K additions, four operations per group flush, the bias add and the lane reduction; for f32 activations also the K
products); the magnitude is q |s| + |b|, not |w|, because the grouped form s sum x q + b sum x can cancel; the factor 2 covers a truncating adder in the matrix
core; u_T |E| is the one rounding to T.  f16 overflow and subnormal handling as `check_bound` of tests/test_zz_blockwise_fp8_gpu.py.  An f32 restatement of the
reference's per-element fma chain (w = fma(q, s, b), acc = fma(x, w, acc) in k order) is held to the same bound on the CPU for the same data."""
import ctypes as C

import numpy as np
import pytest
import torch

import mistralrs_amd  # noqa: F401
from mistralrs_amd import _lib, afq, uqff
from mistralrs_amd.distributed import Shard
from tests.test_afq import BITS, GROUPS, dequantize, dequantize_f64, no_f32_ties, pack, quantize, unpack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
ALL3 = [torch.float32, torch.float16, torch.bfloat16]
IDS3 = ["f32", "f16", "bf16"]
TAG = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
F16_OVERFLOW = 65520.0
PAIRS = [(b, g) for b in BITS for g in GROUPS]


def to_t(a, dtype):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype)


def bits_of(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()


def gpu_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV).view(torch.uint32)


def u32_np(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def check_bound(got, exact, mag, k, group, dtype, what):
    u = U[dtype]
    n_ops = (2 * k if dtype == torch.float32 else k) + 4 * k // group + 4
    b = 2.0 * n_ops * 2.0 ** -24 * mag
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


def f32_tie_mask(v64):
    f = v64.astype(np.float32)
    nb = np.nextafter(f, np.where(v64 > f, np.inf, -np.inf).astype(np.float32))
    return (v64 != f) & (v64 == (f.astype(np.float64) + nb.astype(np.float64)) / 2)


# ------------------------------------------------------------------------------------------------ data
def exact_parts(n, k, bits, group, dtype, e=0):
    """an asymmetric code pattern in n and k, scales in {0.5, 1, 2}, biases -2^(bits - 1) scale or small halves and integers: all exact in every T"""
    nn, kk = np.arange(n)[:, None], np.arange(k)[None, :]
    codes = ((3 * nn + 5 * kk + (nn * kk) // 7 + 11 * e) % (1 << bits)).astype(np.uint32)
    gi = np.arange(k // group)[None, :]
    s = 2.0 ** ((3 * nn + gi + e) % 3 - 1)
    b = np.where((nn + gi) % 2 == 0, -(2.0 ** (bits - 1)) * s, ((nn + 2 * gi + e) % 5 - 2) * 0.5)
    return pack(codes, bits), to_t(s, dtype), to_t(b, dtype)


def random_parts(rng, shape, bits, group, dtype):
    codes = rng.integers(0, 1 << bits, shape, dtype=np.uint32)
    gshape = (*shape[:-1], shape[-1] // group)
    s = to_t(rng.uniform(0.5, 2.0, gshape) * 2.0 ** rng.integers(-8, -3, gshape), dtype)
    b = to_t(-rng.uniform(0.2, 0.8, gshape) * (1 << bits) * s.double().numpy(), dtype)
    return pack(codes, bits), s, b


def oracle(x64, w_q, s, b, bits, group, bias64=None):
    """E and the bound's magnitude for x64 [M, K] against one [N, ..] weight"""
    q = unpack(w_q, bits).astype(np.float64)
    sf, bf = np.repeat(s.double().numpy(), group, -1), np.repeat(b.double().numpy(), group, -1)
    exact = x64 @ (q * sf + bf).T
    mag = np.abs(x64) @ (q * np.abs(sf) + np.abs(bf)).T
    if bias64 is not None:
        exact, mag = exact + bias64, mag + np.abs(bias64)
    return exact, mag


def reference_chain_f32(x, w_q, s, b, bits, group):
    """f32 restatement of the reference GEMV's per-element chain: w = fma(q, s, b) rounded to f32, acc = fma(x_k, w_k, acc) for k ascending"""
    w = dequantize_f64(w_q, s, b, bits, group).astype(np.float32)  # exact f64 -> one f32 rounding = fmaf
    acc = np.zeros((x.shape[0], w.shape[0]), np.float64)
    for k in range(x.shape[1]):
        acc = (acc + x[:, k:k + 1].astype(np.float64) * w[None, :, k].astype(np.float64)).astype(np.float32).astype(np.float64)  # f32 x f32 is exact in f64
    return acc


# ------------------------------------------------------------------------------------------------ dequantize, embedding, quantize
@pytest.mark.parametrize("dtype", ALL3, ids=IDS3)
def test_dequantize_and_embedding_bit_exact(dtype):
    rng = np.random.default_rng(1)
    for bits, group in PAIRS:
        for rows, k in [(3, group), (5, 3 * group)] + ([(9, 96)] if group == 32 else []):
            w_q, s, b = random_parts(rng, (rows, k), bits, group, dtype)
            if dtype == torch.float32:  # keep every f64 value off the f32 ties: step a code that sits on one to the next code
                for _ in range(16):
                    ties = f32_tie_mask(dequantize_f64(w_q, s, b, bits, group))
                    if not ties.any():
                        break
                    w_q = pack((unpack(w_q, bits) + ties.astype(np.uint32)) % (1 << bits), bits)
                assert no_f32_ties(dequantize_f64(w_q, s, b, bits, group))
            want = dequantize(w_q, s, b, bits, group)
            layer = afq.AfqLayer.from_parts(gpu_u32(w_q), s.to(DEV), b.to(DEV), None, bits, group)
            got = layer.dequantize_w()
            assert got.dtype == dtype and np.array_equal(bits_of(got), bits_of(want)), (bits, group, rows, k)
            ids = torch.tensor([[rows - 1, 0], [rows - 1, 1 % rows]])
            emb = layer.embedding_forward(ids.to(DEV))
            assert tuple(emb.shape) == (2, 2, k) and np.array_equal(bits_of(emb), bits_of(want[ids.reshape(-1)].reshape(2, 2, k))), (bits, group, rows, k)
    with pytest.raises(ValueError, match="Embedding id 9 is out of range for 3 rows."):
        afq.AfqLayer.from_parts(gpu_u32(np.zeros((3, 4), np.uint32)), torch.zeros(3, 1, device=DEV), torch.zeros(3, 1, device=DEV), None, 4, 32).embedding_forward(
            torch.tensor([9], device=DEV))


def quant_input(rng, rows, k, group):
    w = (rng.standard_normal((rows, k)) * 0.7).astype(np.float32)
    w[0, :group] = 0.375                                      # a constant group
    w[1, :group] = -0.0                                       # a constant group of negative zeros
    w[2, 1], w[2, 2], w[2, 3] = 0.0, -0.0, -1.5              # signed zeros away from the minimum
    w[rows - 1, :group] = 1e-7
    w[rows - 1, 1] = 3e-7                                     # a range whose scale underflows in f16
    return w


@pytest.mark.parametrize("dtype", ALL3, ids=IDS3)
def test_quantize_bit_exact(dtype):
    rng = np.random.default_rng(2)
    for bits, group in PAIRS:
        for rows, k in [(3, group), (5, 3 * group)] + ([(9, 96)] if group == 32 else []):
            w = torch.from_numpy(quant_input(rng, rows, k, group)).to(dtype)
            want_q, want_s, want_b = quantize(w, bits, group)
            buf = torch.empty(w.numel() + 1, dtype=dtype, device=DEV)  # the input starts one element past the allocation's alignment
            buf[1:] = w.reshape(-1).to(DEV)
            got_q, got_s, got_b = afq.quantize_tensors(buf[1:].view(rows, k), bits, group)
            what = (bits, group, rows, k)
            assert np.array_equal(bits_of(got_s), bits_of(want_s)) and np.array_equal(bits_of(got_b), bits_of(want_b)), what
            bad = np.argwhere(unpack(u32_np(got_q), bits) != unpack(want_q, bits))
            assert not len(bad), f"{what}: {len(bad)} codes differ, first at {tuple(bad[0])}"
            assert np.array_equal(u32_np(got_q), want_q), what
            layer = afq.AfqLayer.quantize(w.to(DEV), None, bits, group)
            assert np.array_equal(bits_of(layer.dequantize_w()), bits_of(dequantize(want_q, want_s, want_b, bits, group))), what


# ------------------------------------------------------------------------------------------------ dense
MS, NS = [1, 2, 7, 8, 9, 33, 65], [1, 9, 129]


def ks_of(group):
    return [group, 3 * group] + ([96] if group == 32 else []) + [2048 + group]


def want_route(m, dtype):
    return 1 if m <= 8 else (5 if dtype == torch.float32 else 2)


@pytest.mark.parametrize("dtype", ALL3, ids=IDS3)
def test_dense_exact_integer(dtype):
    rng = np.random.default_rng(3)
    case = 0
    for pi, (bits, group) in enumerate(PAIRS):
        for mi, m in enumerate(MS):
            for ni, n in enumerate(NS):
                for ki, k in enumerate(ks_of(group)):
                    if m > 8 and (pi + mi + ni + ki) % 2:  # routes 2 and 5: a covering half of the grid; route 1: every case
                        continue
                    if k > 2048 and (pi + mi + ni) % 3:    # the long K on a third of the cases
                        continue
                    case += 1
                    with_bias = case % 2 == 0
                    w_q, s, b = exact_parts(n, k, bits, group, dtype)
                    x = rng.integers(-4, 5, (m, k)).astype(np.float64)
                    bias = ((np.arange(n) % 7) - 3) * 0.5 if with_bias else None
                    exact, _ = oracle(x, w_q, s, b, bits, group, bias)
                    got = afq.matmul(to_t(x, dtype).to(DEV), gpu_u32(w_q), s.to(DEV), b.to(DEV), bits, group, to_t(bias, dtype).to(DEV) if with_bias else None)
                    assert afq.last_route() == want_route(m, dtype), (m, afq.last_route())
                    assert np.array_equal(bits_of(got), bits_of(to_t(exact, dtype))), f"bits {bits} group {group} M {m} N {n} K {k} bias {with_bias}"
    assert case > 300


@pytest.mark.parametrize("dtype", ALL3, ids=IDS3)
def test_dense_random(dtype):
    rng = np.random.default_rng(4)
    for pi, (bits, group) in enumerate(PAIRS):
        for mi, (m, n) in enumerate([(1, 9), (8, 129), (9, 129), (65, 9)]):
            k = ks_of(group)[(pi + mi) % len(ks_of(group))]
            w_q, s, b = random_parts(rng, (n, k), bits, group, dtype)
            tx = to_t(rng.standard_normal((m, k)), dtype)
            bias = to_t(rng.uniform(-1, 1, n), dtype) if mi % 2 else None
            x = tx.double().numpy()
            exact, mag = oracle(x, w_q, s, b, bits, group, None if bias is None else bias.double().numpy())
            got = afq.matmul(tx.to(DEV), gpu_u32(w_q), s.to(DEV), b.to(DEV), bits, group, None if bias is None else bias.to(DEV))
            assert afq.last_route() == want_route(m, dtype)
            what = f"dense {TAG[dtype]} bits {bits} group {group} M {m} N {n} K {k}"
            check_bound(got.float().cpu().numpy(), exact, mag, k, group, dtype, what)
            if m <= 8 and k <= 512:  # the reference formulation sits inside the same bound (CPU)
                ref = reference_chain_f32(tx.float().numpy(), w_q, s, b, bits, group) + (0.0 if bias is None else bias.double().numpy())
                check_bound(to_t(ref, dtype).float().numpy(), exact, mag, k, group, dtype, "reference chain, " + what)


@pytest.mark.parametrize("dtype", ALL3, ids=IDS3)
def test_gemv_rows_do_not_depend_on_m(dtype):
    rng = np.random.default_rng(5)
    for bits, group, k in [(3, 32, 96), (4, 64, 2048 + 64), (6, 128, 384)]:
        w_q, s, b = random_parts(rng, (41, k), bits, group, dtype)
        tw, ts, tb = gpu_u32(w_q), s.to(DEV), b.to(DEV)
        tx = to_t(rng.standard_normal((8, k)), dtype).to(DEV)
        whole = afq.matmul(tx, tw, ts, tb, bits, group)
        assert afq.last_route() == 1
        rows = torch.cat([afq.matmul(tx[i:i + 1], tw, ts, tb, bits, group) for i in range(8)], 0)
        assert np.array_equal(bits_of(whole), bits_of(rows))
        for m in (3, 5, 7):
            assert np.array_equal(bits_of(afq.matmul(tx[:m], tw, ts, tb, bits, group)), bits_of(whole[:m]))


# ------------------------------------------------------------------------------------------------ MoE
E, TOPK, MOE_N, SENTINEL = 4, 2, 129, 7.0


def moe_indices(rng, t):
    idx = rng.integers(0, E - 1, (t, TOPK))  # expert 3 is never chosen
    idx[t // 2, TOPK - 1] = E + 1            # outside the expert range: its output row keeps the sentinel
    return idx


@pytest.mark.parametrize("tokens", [1, 3, 5, 40])
@pytest.mark.parametrize("dtype", ALL3, ids=IDS3)
@pytest.mark.parametrize("exact_ints", [True, False], ids=["exact", "random"])
def test_moe(tokens, dtype, exact_ints):
    rng = np.random.default_rng(tokens * 10 + exact_ints)
    for bits, group, k in [(3, 32, 96), (4, 64, 192), (8, 128, 256), (6, 32, 160), (2, 64, 128)]:
        if exact_ints:
            parts = [exact_parts(MOE_N, k, bits, group, dtype, e) for e in range(E)]
        else:
            parts = [random_parts(rng, (MOE_N, k), bits, group, dtype) for _ in range(E)]
        w_q, s, b = np.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), torch.stack([p[2] for p in parts])
        ebias = to_t(((np.arange(E)[:, None] + np.arange(MOE_N)[None, :]) % 5 - 2) * 0.5 if exact_ints else rng.uniform(-1, 1, (E, MOE_N)), dtype)
        layer = afq.AfqLayer.from_parts(gpu_u32(w_q), s.to(DEV), b.to(DEV), ebias.to(DEV), bits, group)
        idx = moe_indices(rng, tokens)
        tidx = torch.from_numpy(idx.astype(np.int32)).to(DEV)
        route = 4 if tokens * TOPK > 8 and dtype != torch.float32 else 3
        for rank in (2, 3):
            shape = (tokens, k) if rank == 2 else (tokens, TOPK, k)
            tx = to_t(rng.integers(-4, 5, shape) if exact_ints else rng.standard_normal(shape), dtype)
            x3 = tx.double().numpy() if rank == 3 else np.repeat(tx.double().numpy()[:, None], TOPK, 1)
            exact, mag = np.full((tokens, TOPK, MOE_N), SENTINEL), np.zeros((tokens, TOPK, MOE_N))
            skipped = np.zeros((tokens, TOPK, MOE_N), bool)
            for i in range(tokens):
                for sl in range(TOPK):
                    e = int(idx[i, sl])
                    if e < E:
                        ex, mg = oracle(x3[i, sl][None], w_q[e], s[e], b[e], bits, group, ebias[e].double().numpy())
                        exact[i, sl], mag[i, sl] = ex[0], mg[0]
                    else:
                        skipped[i, sl] = True
            assert skipped.sum() == MOE_N
            out = torch.full((tokens, TOPK, MOE_N), SENTINEL, dtype=dtype, device=DEV)
            got = afq.indexed_moe_gemm(tx.to(DEV), layer.w_q, layer.scales, layer.biases, bits, group, tidx, layer.bias, out=out)
            assert afq.last_route() == route, (tokens, afq.last_route())
            what = f"moe {TAG[dtype]} T {tokens} bits {bits} group {group} K {k} x rank {rank}"
            if exact_ints:
                assert np.array_equal(bits_of(got), bits_of(to_t(exact, dtype))), what
            else:
                g = got.float().cpu().numpy()
                assert np.all(g[skipped] == SENTINEL), what
                check_bound(g, exact, mag, k, group, dtype, what)
            if tokens <= 3 and rank == 2:  # both on the GEMV: gather_forward is the per-slot forward on the selected expert
                ok_idx = np.where(idx < E, idx, 0)
                y = layer.gather_forward(tx.to(DEV), torch.from_numpy(ok_idx.astype(np.int64)).to(DEV))
                assert afq.last_route() == 3
                for i in range(tokens):
                    for sl in range(TOPK):
                        e = int(ok_idx[i, sl])
                        one = afq.AfqLayer.from_parts(layer.w_q[e], layer.scales[e], layer.biases[e], layer.bias[e], bits, group).forward(tx[i:i + 1].to(DEV))
                        assert afq.last_route() == 1 and np.array_equal(bits_of(y[i, sl]), bits_of(one[0])), what


# ------------------------------------------------------------------------------------------------ the reference's C symbols
def test_reference_symbols_match_native_entry_points():
    rng = np.random.default_rng(7)
    dt, lib = torch.bfloat16, _lib.load("quant")
    p = lambda t: C.c_void_p(t.data_ptr())

    def parts(bits, group, n, k):
        w_q, s, b = random_parts(rng, (n, k), bits, group, dt)
        return gpu_u32(w_q), s.to(DEV), b.to(DEV)

    for name, bits, group, m in (("afq_qmv_4bit_gs64_bf16", 4, 64, 3), ("afq_qmm_8bit_gs32_bf16", 8, 32, 33), ("afq_qmv_6bit_gs128_bf16", 6, 128, 20)):
        tw, ts, tb = parts(bits, group, 41, 384)
        tx = to_t(rng.standard_normal((m, 384)), dt).to(DEV)
        want = afq.matmul(tx, tw, ts, tb, bits, group)
        route = afq.last_route()
        y = torch.zeros(m, 41, dtype=dt, device=DEV)
        torch.cuda.synchronize()
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [C.c_void_p] * 5 + [C.c_int] * 3, None
        fn(p(tx), p(tw), p(ts), p(tb), p(y), m, 41, 384)
        torch.cuda.synchronize()
        assert afq.last_route() == route and np.array_equal(bits_of(y), bits_of(want)), name
    tw, ts, tb = parts(3, 32, 9, 96)
    layer = afq.AfqLayer.from_parts(tw, ts, tb, None, 3, 32)
    out = torch.zeros(9, 96, dtype=dt, device=DEV)
    torch.cuda.synchronize()
    fn = lib.afq_dequantize_3bit_gs32_bf16
    fn.argtypes, fn.restype = [C.c_void_p] * 4 + [C.c_int] * 2, None
    fn(p(tw), p(ts), p(tb), p(out), 9, 96)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(out), bits_of(layer.dequantize_w()))
    tw, ts, tb = parts(6, 64, 9, 192)
    layer = afq.AfqLayer.from_parts(tw, ts, tb, None, 6, 64)
    ids = torch.tensor([8, 2, 8, 0], dtype=torch.int32, device=DEV)
    out = torch.zeros(4, 192, dtype=dt, device=DEV)
    torch.cuda.synchronize()
    fn = lib.afq_embedding_6bit_gs64_bf16
    fn.argtypes, fn.restype = [C.c_void_p] * 5 + [C.c_int] * 2, None
    fn(p(tw), p(ts), p(tb), p(ids), p(out), 4, 192)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(out), bits_of(layer.embedding_forward(ids)))
    w = to_t(rng.standard_normal((5, 256)), torch.float16).to(DEV)
    want_q, want_s, want_b = afq.quantize_tensors(w, 2, 128)
    q, s, b = torch.zeros(5, 16, dtype=torch.int32, device=DEV), torch.zeros(5, 2, dtype=torch.float16, device=DEV), torch.zeros(5, 2, dtype=torch.float16, device=DEV)
    torch.cuda.synchronize()
    fn = lib.afq_quantize_2bit_gs128_f16
    fn.argtypes, fn.restype = [C.c_void_p] * 4 + [C.c_int] * 2, None
    fn(p(w), p(q), p(s), p(b), 5, 256)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(q), bits_of(want_q)) and np.array_equal(bits_of(s), bits_of(want_s)) and np.array_equal(bits_of(b), bits_of(want_b))


# ------------------------------------------------------------------------------------------------ the layer, UQFF end to end
def test_layer_uqff_sharded_forward(tmp_path):
    rng = np.random.default_rng(8)
    n, k, bits, group, dt = 41, 384, 3, 64, torch.bfloat16
    w = to_t(rng.standard_normal((n, k)), dt).to(DEV)
    bias = to_t(rng.uniform(-1, 1, n), dt).to(DEV)
    layer = afq.AfqLayer.quantize(w, bias, bits, group)
    assert layer.uqff_type() == "AFQ3" and layer.has_bias() and layer.dtype_and_device()[0] == dt and layer.apply_isq("AFQ3") is layer
    path = str(tmp_path / "l.uqff")
    uqff.write(path, layer.serialize_uqff("l"))
    r = uqff.UqffReader(path)
    back = afq.AfqLayer.from_uqff(r, "l", DEV)
    x = to_t(rng.standard_normal((2, 3, k)), dt).to(DEV)
    y = layer.forward(x)
    assert tuple(y.shape) == (2, 3, n) and np.array_equal(bits_of(back.forward(x)), bits_of(y))
    for rank in range(2):  # a world-2 shard of the input dim: the sliced layer, without the bias (the caller adds it after the all-reduce)
        part = afq.AfqLayer.from_uqff(r, "l", DEV, Shard(dim=1, rank=rank, world_size=2))
        cols = slice(rank * k // 2, (rank + 1) * k // 2)
        words = slice(rank * k // 2 * bits // 32, (rank + 1) * k // 2 * bits // 32)
        groups = slice(rank * k // 2 // group, (rank + 1) * k // 2 // group)
        sliced = afq.AfqLayer.from_parts(layer.w_q[:, words].contiguous(), layer.scales[:, groups].contiguous(), layer.biases[:, groups].contiguous(), None, bits, group)
        assert part.bias is None and np.array_equal(bits_of(part.forward(x[..., cols])), bits_of(sliced.forward(x[..., cols])))
    # requantize to a GGML type through the dense weight, and add_delta_w
    from mistralrs_amd.gguf.matmul import GgufMatMul
    from mistralrs_amd.gguf.qtensor import GgmlDType
    got = afq.AfqLayer.quantize(w[:, :256].contiguous(), None, 4, 64).apply_isq(GgmlDType.Q8_0)
    assert isinstance(got, GgufMatMul) and got.w.dtype == GgmlDType.Q8_0
    moved = layer.add_delta_w(torch.zeros_like(w))
    assert moved.bits == bits and moved.group_size == group and tuple(moved.w_q.shape) == tuple(layer.w_q.shape)
