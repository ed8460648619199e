"""GPU: the GPTQ / AWQ kernels (reconstruct, AWQ repack, matmul on routes 1 / 2), the reference's C symbols and `GptqLayer` against the numpy oracle of
tests/test_gptq.py.  Reconstruct, `dequantize_w` and the repack are compared bit for bit, and so are the exact-integer matmul cases: every product and every
partial sum is an exact f32 and the result is exactly representable in f16 (asserted on the CPU), so any summation order must give f16(exact).  Random
cases are held, element by element and with no exclusions, to

    |got - E| <= B (1 + 2^-11) + 2^-11 |E|,   B = 2 (K + 4) 2^-24 (sum_k |x_k| |W_kn| + |bias_n|)

with E the f64 value of sum_k x_k W_kn + bias_n at the oracle's f16 W.  W is already rounded, a product of two f16 values is exact in f32, so (K + 4) 2^-24
bounds the f32 roundings on the way of a term (K additions, the reduction across waves, the bias add); the factor 2 covers a truncating adder in the matrix
core; 2^-11 |E| is the one rounding to f16.  The inputs keep |E| + B below 65504 (asserted).  An f32 restatement of "reconstruct, then a k-ordered fma chain"
is held to the same bound on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import mistralrs_amd  # noqa: F401
from mistralrs_amd import _lib, gptq
from tests.test_gptq import (BITS, GROUPS, awq_dequantize, awq_interleave, awq_repack, pack_k, pack_n, reconstruct)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(b, g) for b in BITS for g in GROUPS]
SENTINEL = -777.0
F16_MAX = 65504.0


def gpu_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def gpu_f16(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float16))).to(DEV)


def bits_of(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def np_bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float16)).view(np.int16)


def u32_np(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def g_idx_of(kind, k, group, rng):
    """sequential; a permutation with equal group counts (act-order); an arbitrary map with unequal counts"""
    g = k // group
    seq = (np.arange(k) // group).astype(np.int32)
    if kind == "seq":
        return seq
    if kind == "perm":
        return seq[rng.permutation(k)]
    gi = rng.integers(0, g, k).astype(np.int32)
    gi[: min(k, 5)] = g - 1  # a short run, then a change inside a 32-row unit
    return gi


def on_gpu(parts):
    qw, qz, sc, gi = parts
    return gpu_i32(qw), gpu_i32(qz), gpu_f16(sc), gpu_i32(gi)


def shapes_of(group):
    return [(group, 32), (3 * group, 96)] + ([(96, 160)] if group == 32 else [])


# ------------------------------------------------------------------------------------------------ reconstruct, dequantize_w
def random_parts(rng, k, n, bits, group, kind, edge_scales=False):
    top = (1 << bits) - 1
    g = k // group
    codes = rng.integers(0, top + 1, (k, n), dtype=np.uint32)
    zeros = rng.integers(0, top + 1, (g, n), dtype=np.uint32)
    gi = g_idx_of(kind, k, group, rng)
    zeros[0, 0], zeros[0, 1], zeros[g - 1, n - 1] = 0, top, top
    for grp, col in ((0, 0), (0, 1), (g - 1, n - 1)):  # both ends of the code range against stored zeros 0 and 2^bits - 1: q - z - 1 from -2^bits to 2^bits - 2
        rows = np.flatnonzero(gi == grp)
        if len(rows):
            codes[rows[0], col], codes[rows[-1], col] = top, 0
    sc = (rng.uniform(0.5, 2.0, (g, n)) * 2.0 ** rng.integers(-8, -3, (g, n))).astype(np.float16)
    if edge_scales:
        sc[0, 0], sc[0, 1], sc[g - 1, n - 1], sc[0, 2] = 2.0 ** -20, 65504.0 / 256.0, 65504.0 / 256.0, 3 * 2.0 ** -24  # two f16 subnormals, the largest safe scale
    return pack_k(codes, bits), pack_n(zeros, bits), sc, gi


@pytest.mark.parametrize("bits", BITS)
def test_reconstruct_and_dequantize_w_bit_exact(bits):
    rng = np.random.default_rng(10 + bits)
    for group in GROUPS:
        for k, n in shapes_of(group):
            for kind in ("seq", "perm", "unequal"):
                parts = random_parts(rng, k, n, bits, group, kind, edge_scales=True)
                want = reconstruct(*parts, bits, 1)
                assert np.isfinite(want.astype(np.float64)).all()  # |q - z - 1| <= 256 times 65504 / 256 stays finite
                t = on_gpu(parts)
                out = torch.full((k, n), SENTINEL, dtype=torch.float16, device=DEV)
                got = gptq.reconstruct(*t, bits, 1, out=out)
                what = (bits, group, k, n, kind)
                assert np.array_equal(bits_of(got), np_bits(want)), what
                layer = gptq.GptqLayer.from_parts(*t, None, bits)
                w = layer.dequantize_w()
                assert tuple(w.shape) == (n, k) and w.is_contiguous() and np.array_equal(bits_of(w), np_bits(want.T)), what
                if kind == "seq":  # the other zero offset on the same tensors
                    assert np.array_equal(bits_of(gptq.reconstruct(*t, bits, 0)), np_bits(reconstruct(*parts, bits, 0))), what


# ------------------------------------------------------------------------------------------------ AWQ repack
def awq_parts(rng, k, n, bits, group):
    top = (1 << bits) - 1
    g = k // group
    codes = rng.integers(0, top + 1, (k, n), dtype=np.uint32)
    zeros = rng.integers(0, top + 1, (g, n), dtype=np.uint32)
    zeros[0, :3] = [0, top, 1]  # a true zero point of 0
    sc = (rng.uniform(0.5, 2.0, (g, n)) * 2.0 ** rng.integers(-8, -3, (g, n))).astype(np.float16)
    return awq_interleave(codes, bits), awq_interleave(zeros, bits), sc


@pytest.mark.parametrize("bits", [4, 8])
def test_awq_repack_bit_exact(bits):
    rng = np.random.default_rng(20 + bits)
    for group in GROUPS:
        for k, n in shapes_of(group):
            qw_a, qz_a, sc = awq_parts(rng, k, n, bits, group)
            want_qw, want_qz, want_gi = awq_repack(qw_a, qz_a, bits, group)
            qw, qz, gi = gptq.awq_repack(gpu_i32(qw_a), gpu_i32(qz_a), bits, group)
            what = (bits, group, k, n)
            assert np.array_equal(u32_np(qw), want_qw) and np.array_equal(u32_np(qz), want_qz) and np.array_equal(gi.cpu().numpy(), want_gi), what
            layer = gptq.GptqLayer.from_parts(gpu_i32(qw_a), gpu_i32(qz_a), gpu_f16(sc), None, None, bits, is_awq=True)
            assert layer.is_awq and layer.zero_offset == 0 and layer.group_size == group
            assert np.array_equal(bits_of(layer.dequantize_w()), np_bits(awq_dequantize(qw_a, qz_a, sc, bits, group).T)), what


# ------------------------------------------------------------------------------------------------ dense, exact integers
MS, NS = [1, 2, 7, 8, 9, 33, 65], [32, 96, 160]


def ks_of(group):
    return [group, 3 * group, 2048 + group]


def exact_codes(rng, k, n, bits, group, off, gi):
    """stored zeros over the whole range (0 and 2^bits - 1 included), codes within two steps of the zero point so that the sums stay small, scales in {0.5, 1, 2}"""
    top = (1 << bits) - 1
    g = k // group
    zeros = rng.integers(0, top + 1, (g, n), dtype=np.uint32)
    zeros[0, 0], zeros[0, 1] = 0, top
    d = rng.integers(-2, 3, (k, n))
    codes = np.clip(zeros.astype(np.int64)[gi] + off + d, 0, top).astype(np.uint32)
    sc = (2.0 ** rng.integers(-1, 2, (g, n))).astype(np.float16)
    return codes, zeros, sc


def exact_x(rng, m, k):
    """integers in [-4, 4]; past 512 columns three in four are zero so that the exact sums stay representable in f16"""
    x = rng.integers(-4, 5, (m, k)).astype(np.float64)
    if k > 512:
        x *= rng.random((m, k)) < 0.25
        x[:, 0], x[:, k - 1] = 3.0, -2.0
    return x


def f16_exact(v):
    with np.errstate(over="ignore"):
        return np.array_equal(v.astype(np.float16).astype(np.float64), v)


@pytest.mark.parametrize("bits", BITS)
def test_dense_exact_integer(bits):
    rng = np.random.default_rng(30 + bits)
    case = n_awq = n_offset = 0
    kinds = set()
    for gi_, group in enumerate(GROUPS):
        for ni, n in enumerate(NS):
            for ki, k in enumerate(ks_of(group)):
                awq = bits in (4, 8) and (gi_ + ni + ki) % 3 == 0
                kind = "seq" if awq else ("seq", "perm")[(gi_ + ni + ki) % 2]
                kinds.add(kind)
                gi = g_idx_of(kind, k, group, rng)
                off = 0 if awq else 1
                codes, zeros, sc = exact_codes(rng, k, n, bits, group, off, gi)
                w64 = reconstruct(pack_k(codes, bits), pack_n(zeros, bits), sc, gi, bits, off).astype(np.float64)
                if awq:
                    n_awq += 1
                    layer = gptq.GptqLayer.from_parts(gpu_i32(awq_interleave(codes, bits)), gpu_i32(awq_interleave(zeros, bits)), gpu_f16(sc), None, None, bits, is_awq=True)
                    t = (layer.qweight, layer.qzeros, layer.scales, layer.g_idx)
                else:
                    t = on_gpu((pack_k(codes, bits), pack_n(zeros, bits), sc, gi))
                for mi, m in enumerate(MS):
                    if m > 8 and (gi_ + ni + ki + mi) % 2:  # route 2: a covering half of the grid; route 1: every case
                        continue
                    case += 1
                    with_bias = case % 2 == 0
                    x = exact_x(rng, m, k)
                    bias = ((np.arange(n) % 7) - 3) * 0.5 if with_bias else None
                    exact = x @ w64 + (0.0 if bias is None else bias)
                    what = f"bits {bits} group {group} M {m} N {n} K {k} g_idx {kind} awq {awq} bias {with_bias}"
                    # CPU: every partial sum is an exact f32 and the result is an f16 value, so the definition alone gives these bits
                    assert float((np.abs(x) @ np.abs(w64)).max()) + 2.0 < 2.0 ** 24 and f16_exact(exact), what
                    if m in (7, 33) and ni == 1:  # x starts one element into its allocation: 2-byte aligned only
                        n_offset += 1
                        buf = torch.empty(m * k + 1, dtype=torch.float16, device=DEV)
                        buf[1:] = gpu_f16(x).reshape(-1)
                        tx = buf[1:].view(m, k)
                        assert tx.data_ptr() % 4 == 2 and tx.is_contiguous()
                    else:
                        tx = gpu_f16(x)
                    out = torch.full((m, n), SENTINEL, dtype=torch.float16, device=DEV)
                    got = gptq.matmul(tx, *t, bits, None if bias is None else gpu_f16(bias), off, out=out)
                    assert gptq.last_route() == (1 if m <= 8 else 2), (m, gptq.last_route())
                    assert np.array_equal(bits_of(got), np_bits(exact)), what
    assert case >= 27 * 5 and kinds == {"seq", "perm"} and n_offset >= 2 and (n_awq > 0) == (bits in (4, 8))


# ------------------------------------------------------------------------------------------------ dense, random
def check_bound(got, exact, mag, k, what):
    u = 2.0 ** -11
    b = 2.0 * (k + 4) * 2.0 ** -24 * mag
    assert float((np.abs(exact) + b).max()) < F16_MAX, what  # nothing near the overflow threshold
    got = got.astype(np.float64)
    lim = b * (1 + u) + u * np.abs(exact)
    err = np.abs(got - exact)
    worst = float(np.max(err / np.maximum(lim, 1e-300)))
    print(f"{what}: worst error / bound = {worst:.3f}")
    bad = np.argwhere(~(err <= lim))
    assert not len(bad), (f"{what}: {len(bad)} of {err.size} elements outside the bound (worst {worst:.2f}x); first at {tuple(bad[0])}: "
                          f"got {got[tuple(bad[0])]!r} exact {exact[tuple(bad[0])]!r} bound {lim[tuple(bad[0])]!r}")


def reference_chain_f32(x16, w16, bias16):
    """f32 restatement of "reconstruct, then a k-ordered fma chain": acc = fma(x_k, W_kn, acc) for k ascending, the bias added in f32, one rounding to f16"""
    x, w = x16.astype(np.float64), w16.astype(np.float64)
    acc = np.zeros((x.shape[0], w.shape[1]), np.float64)
    for k in range(x.shape[1]):
        acc = (acc + x[:, k:k + 1] * w[k:k + 1, :]).astype(np.float32).astype(np.float64)  # f16 x f16 is exact, the sum rounds once: fmaf
    if bias16 is not None:
        acc = (acc + bias16.astype(np.float64)).astype(np.float32).astype(np.float64)
    return acc.astype(np.float16)


@pytest.mark.parametrize("bits", BITS)
def test_dense_random(bits):
    rng = np.random.default_rng(40 + bits)
    for gi_, group in enumerate(GROUPS):
        for mi, (m, n) in enumerate([(1, 32), (8, 160), (9, 160), (65, 96)]):
            k = ks_of(group)[(gi_ + mi) % 3]
            kind = ("perm", "seq", "unequal")[(gi_ + mi) % 3]
            parts = random_parts(rng, k, n, bits, group, kind)
            w16 = reconstruct(*parts, bits, 1)
            x16 = rng.standard_normal((m, k)).astype(np.float16)
            bias16 = rng.uniform(-1, 1, n).astype(np.float16) if mi % 2 else None
            x, w = x16.astype(np.float64), w16.astype(np.float64)
            exact, mag = x @ w, np.abs(x) @ np.abs(w)
            if bias16 is not None:
                exact, mag = exact + bias16.astype(np.float64), mag + np.abs(bias16.astype(np.float64))
            out = torch.full((m, n), SENTINEL, dtype=torch.float16, device=DEV)
            got = gptq.matmul(gpu_f16(x16), *on_gpu(parts), bits, None if bias16 is None else gpu_f16(bias16), out=out)
            assert gptq.last_route() == (1 if m <= 8 else 2)
            what = f"dense bits {bits} group {group} M {m} N {n} K {k} g_idx {kind}"
            check_bound(got.float().cpu().numpy(), exact, mag, k, what)
            if k <= 512:  # the reference formulation sits inside the same bound (CPU)
                check_bound(reference_chain_f32(x16, w16, bias16).astype(np.float32), exact, mag, k, "reference chain, " + what)


# ------------------------------------------------------------------------------------------------ determinism
def test_gemv_rows_do_not_depend_on_m():
    rng = np.random.default_rng(5)
    for bits, group, k, n, kind in [(3, 32, 96, 160, "perm"), (4, 128, 2048 + 128, 96, "seq"), (8, 64, 192, 32, "unequal"), (2, 64, 64, 96, "perm")]:
        t = on_gpu(random_parts(rng, k, n, bits, group, kind))
        bias = gpu_f16(rng.uniform(-1, 1, n))
        tx = gpu_f16(rng.standard_normal((8, k)))
        whole = gptq.matmul(tx, *t, bits, bias)
        assert gptq.last_route() == 1
        rows = torch.cat([gptq.matmul(tx[i:i + 1], *t, bits, bias) for i in range(8)], 0)
        assert np.array_equal(bits_of(whole), bits_of(rows)), (bits, group)
        for m in (3, 5, 7):
            assert np.array_equal(bits_of(gptq.matmul(tx[:m], *t, bits, bias)), bits_of(whole[:m])), (bits, group, m)


def test_repeat_launch_gives_identical_bits():
    rng = np.random.default_rng(6)
    for bits, group, k, n in [(4, 128, 2048 + 128, 160), (3, 32, 96, 96)]:
        t = on_gpu(random_parts(rng, k, n, bits, group, "perm"))
        for m, route in ((8, 1), (65, 2)):
            tx = gpu_f16(rng.standard_normal((m, k)))
            a = gptq.matmul(tx, *t, bits, out=torch.full((m, n), SENTINEL, dtype=torch.float16, device=DEV))
            assert gptq.last_route() == route
            b = gptq.matmul(tx, *t, bits, out=torch.zeros(m, n, dtype=torch.float16, device=DEV))
            assert np.array_equal(bits_of(a), bits_of(b)), (bits, m)


# ------------------------------------------------------------------------------------------------ the reference's C symbols
def test_reference_symbols_match_native_entry_points():
    rng = np.random.default_rng(7)
    lib = _lib.load("quant")
    p = lambda t: C.c_void_p(t.data_ptr())
    for bits, group, k, n in [(4, 64, 192, 96), (8, 32, 96, 160), (3, 128, 128, 32)]:
        t = on_gpu(random_parts(rng, k, n, bits, group, "perm"))
        want = gptq.reconstruct(*t, bits, 1)
        out = torch.full((k, n), SENTINEL, dtype=torch.float16, device=DEV)
        torch.cuda.synchronize()
        fn = lib.reconstruct_gptq
        fn.argtypes, fn.restype = [C.c_void_p] * 5 + [C.c_int] * 4, None
        fn(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(out), k, n, k // group, bits)
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(out), bits_of(want)), bits
        if bits == 3:
            continue
        for m in (3, 33):
            tx = gpu_f16(rng.standard_normal((m, k)))
            want = gptq.matmul(tx, *t, bits)
            route = gptq.last_route()
            y = torch.full((m, n), SENTINEL, dtype=torch.float16, device=DEV)
            torch.cuda.synchronize()
            fn = lib.gemm_half_q_half_alt
            fn.argtypes, fn.restype = [C.c_void_p] * 6 + [C.c_int] * 4, None
            fn(p(tx), p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(y), m, n, k, bits)
            torch.cuda.synchronize()
            assert gptq.last_route() == route and np.array_equal(bits_of(y), bits_of(want)), (bits, m)


# ------------------------------------------------------------------------------------------------ the layer
def test_layer_forward_casts_shapes_and_loader():
    rng = np.random.default_rng(8)
    bits, group, k, n = 4, 64, 192, 96
    parts = random_parts(rng, k, n, bits, group, "perm")
    t = on_gpu(parts)
    bias = gpu_f16(rng.uniform(-1, 1, n))
    layer = gptq.GptqLayer.from_parts(*t, bias, bits)
    assert layer.dtype_and_device()[0] == torch.float16 and layer.has_bias()
    for dt in (torch.bfloat16, torch.float32):
        for shape in ((2, 3, k), (20, k), (2, 2, 5, k)):
            x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV).to(dt)
            y = layer.forward(x)
            raw = layer.forward_raw(x.to(torch.float16))
            assert y.dtype == dt and tuple(y.shape) == (*shape[:-1], n) and raw.dtype == torch.float16
            assert torch.equal(y, raw.to(dt))
            flat = gptq.matmul(x.to(torch.float16).reshape(-1, k), *t, bits, bias)
            assert np.array_equal(bits_of(raw.reshape(-1, n)), bits_of(flat))
    with pytest.raises(ValueError, match="forward_raw expects f16 activations"):
        layer.forward_raw(torch.zeros(1, k, device=DEV))
    # the loader, from a dict of CPU tensors
    names = ("qweight", "qzeros", "scales", "g_idx")
    tensors = {f"m.{nm}": v.cpu() for nm, v in zip(names, t)}
    tensors["m.bias"] = bias.cpu()
    loaded = gptq.gptq_linear(k, n, {"quant_method": "gptq", "bits": bits, "group_size": group}, tensors, "m", device=DEV)
    x = gpu_f16(rng.standard_normal((5, k)))
    assert loaded.has_bias() and np.array_equal(bits_of(loaded.forward(x)), bits_of(layer.forward(x)))
    # AWQ: the layer forward equals a GPTQ-layout layer built from the oracle-repacked tensors
    for abits in (4, 8):
        qw_a, qz_a, sc = awq_parts(rng, k, n, abits, group)
        a_layer = gptq.gptq_linear(k, n, {"quant_method": "awq", "bits": abits, "group_size": group},
                                   {"a.qweight": torch.from_numpy(qw_a.view(np.int32)), "a.qzeros": torch.from_numpy(qz_a.view(np.int32)),
                                    "a.scales": torch.from_numpy(sc), "a.bias": bias.cpu()}, "a", device=DEV)
        qw, qz, gi = awq_repack(qw_a, qz_a, abits, group)
        g_layer = gptq.GptqLayer(gpu_i32(qw), gpu_i32(qz), gpu_f16(sc), gpu_i32(gi), bias, abits, zero_offset=0)
        assert a_layer.is_awq and not g_layer.is_awq
        for m in (5, 20):
            x = gpu_f16(rng.standard_normal((m, k)))
            assert np.array_equal(bits_of(a_layer.forward(x)), bits_of(g_layer.forward(x))), (abits, m)
