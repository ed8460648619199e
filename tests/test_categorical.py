"""Device categorical draw over the whole vocabulary (csrc/sampling.hip, reference ABI `categorical_large_f32_packed_batched`): temperature sampling without top-k.
The kernel inverts the cumulative distribution of softmax(x * invT) at one uniform per row.  Checked against EXACT arithmetic (float64), not against another f32
summation tree: a row's token must lie within `eps` of the exact inversion, and must EQUAL it wherever the uniform is more than `eps` away from both ends of the
exact token's interval.  Every body takes a backend of tests/abi_backends.py: the host emulation in the CPU suite, the MI355X under `-m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

VP, I, LL = C.c_void_p, C.c_int, C.c_int64
U_TOP = np.float32(1.0 - 2.0 ** -24)  # the largest f32 below 1
NINF = np.float32(-np.inf)


def run_cat(be, xs, inv_t, us, chunk, nblocks=None):
    """one batched launch: (packed [rows, 2], block_values [rows, nb], block_sums [rows, nb])"""
    xs = np.ascontiguousarray(xs, dtype=np.float32).reshape(len(us), -1)
    rows, n = xs.shape
    nb = (n + chunk - 1) // chunk if nblocks is None else nblocks
    inv_t = np.broadcast_to(np.asarray(inv_t, dtype=np.float32), (rows,))
    xb, tb, ub = be.buf(xs), be.buf(np.ascontiguousarray(inv_t)), be.buf(np.asarray(us, dtype=np.float32))
    bv, bs, pk = be.buf(np.full(rows * nb, 7.0, np.float32)), be.buf(np.full(rows * nb, 7.0, np.float32)), be.buf(np.full(rows * 2, 7.0, np.float32))
    be.sym("categorical_large_f32_packed_batched", [VP, VP, VP, VP, VP, VP, I, I, I, I, LL])(xb.ptr, tb.ptr, ub.ptr, bv.ptr, bs.ptr, pk.ptr, rows, n, chunk, nb, be.stream or 0)
    return pk.numpy().reshape(rows, 2), bv.numpy().reshape(rows, nb), bs.numpy().reshape(rows, nb)


def exact_cdf(x, inv_t):
    """float64 cumulative distribution of softmax(x * inv_t) (inv_t: the f32 value the kernel gets) and the exact log-probabilities"""
    z = x.astype(np.float64) * np.float64(np.float32(inv_t))
    z -= z.max()
    p = np.exp(z)
    return np.cumsum(p) / p.sum(), z - np.log(p.sum())


# ---------------------------------------------------------------- A. exact cases
def _row(n, fill, **at):
    x = np.full(n, fill, np.float32)
    for i, v in at.items():
        x[int(i[1:])] = v
    return x


def check_exact_cases(be):
    a, b = _row(2051, -10.0, i0=0.0, i1=1.0, i2=2.0), _row(2051, -20.0, i2049=4.0)
    pk, bv, bs = run_cat(be, a[None], 1.0, [0.2], 2048)
    assert pk[0, 0] == 1.0, pk
    pk, bv, bs = run_cat(be, b[None], 0.5, [0.5], 2048)
    assert pk[0, 0] == 2049.0, pk  # second chunk, a partial one
    assert bv[0].tolist() == [-20.0, 4.0]
    pk, _, _ = run_cat(be, np.stack([a, b]), [1.0, 0.5], [0.2, 0.5], 2048)
    assert pk[:, 0].tolist() == [1.0, 2049.0], pk
    for x, it, t in ((a, 1.0, 1), (b, 0.5, 2049)):
        np.testing.assert_allclose(pk[0 if t == 1 else 1, 1], exact_cdf(x, it)[1][t], rtol=2e-6, atol=2e-6)
    # the upper-boundary clamp: u * denom rounds to denom itself
    pk, _, bs = run_cat(be, np.zeros((1, 2048), np.float32), 1.0, [U_TOP], 2048)
    assert pk[0, 0] == 2047.0 and bs[0, 0] == 2048.0, (pk, bs)
    np.testing.assert_allclose(pk[0, 1], -np.log(2048.0), rtol=2e-6)
    # zero-weight tokens are never chosen
    z = np.array([NINF, 0, NINF, 0, NINF], np.float32)
    us = [0.0, 0.25, 0.5, 0.75, U_TOP]
    pk, _, _ = run_cat(be, np.tile(z, (5, 1)), 1.0, us, 2048)
    assert pk[:, 0].tolist() == [1.0, 1.0, 3.0, 3.0, 3.0], pk
    np.testing.assert_allclose(pk[:, 1], np.log(0.5), rtol=2e-6)
    pk, _, _ = run_cat(be, np.tile(z, (5, 1)), 1.0, us, 2)  # the same row cut into chunks of two: (-inf, 0) (-inf, 0) (-inf)
    assert pk[:, 0].tolist() == [1.0, 1.0, 3.0, 3.0, 3.0], pk
    # one column
    pk, bv, bs = run_cat(be, np.array([[-3.5]], np.float32), 0.7, [0.99], 2048)
    assert pk[0].tolist() == [0.0, 0.0] and bv[0, 0] == np.float32(-3.5) and bs[0, 0] == 1.0, (pk, bv, bs)
    # more chunks than the row needs: the empty ones report (-inf, 0) and are never selected
    pk, bv, bs = run_cat(be, a[None], 1.0, [U_TOP], 2048, nblocks=4)
    assert pk[0, 0] == 2050.0 and bv[0, 2:].tolist() == [NINF, NINF] and bs[0, 2:].tolist() == [0.0, 0.0], (pk, bv, bs)


def check_invalid_rows(be):
    """each bad row reports (NaN, NaN); the good rows between them are what they are alone"""
    n = 2051
    good = _row(n, -10.0, i0=0.0, i1=1.0, i2=2.0)
    with_nan, with_inf, all_ninf = good.copy(), good.copy(), np.full(n, NINF, np.float32)
    with_nan[2050] = np.nan
    with_inf[7] = np.inf
    rows = [good, with_nan, good, with_inf, all_ninf, good, good, good, good, good, good]
    inv_t = [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, -1.0, np.inf, 1.0]
    us = [0.2, 0.2, 0.9, 0.2, 0.2, 0.2, 1.0, -0.1, 0.2, 0.2, np.nan]
    bad = [1, 3, 4, 5, 6, 7, 8, 9, 10]
    pk, bv, bs = run_cat(be, np.stack(rows), inv_t, us, 2048)
    for r in range(len(rows)):
        if r in bad:
            assert np.isnan(pk[r]).all(), (r, pk[r])
        else:
            alone, _, _ = run_cat(be, rows[r][None], inv_t[r], [us[r]], 2048)
            np.testing.assert_array_equal(pk[r].view(np.uint32), alone[0].view(np.uint32))
            assert np.isfinite(pk[r]).all()
    assert pk[0, 0] == 1.0 and pk[2, 0] == 2.0
    # the workspace contract on the odd chunks: a NaN chunk reports (NaN, NaN), a chunk of -inf (-inf, 0); the NaN stays inside its chunk
    assert bv[1, 0] == 2.0 and np.isnan(bv[1, 1]) and np.isnan(bs[1, 1]) and np.isfinite(bs[1, 0])
    assert bv[4].tolist() == [NINF, NINF] and bs[4].tolist() == [0.0, 0.0]


def check_launcher_refuses(be):
    """shapes outside the launcher return without launching: the output keeps what the caller left in it"""
    x = np.zeros((1, 100), np.float32)
    for chunk, nb in ((0, 1), (4097, 1), (10, 9)):
        pk, _, _ = run_cat(be, x, 1.0, [0.5], chunk, nblocks=nb)
        assert pk[0].tolist() == [7.0, 7.0], (chunk, nb, pk)
    pk, _, _ = run_cat(be, x, 1.0, [0.5], 4096)
    assert pk[0, 0] == 50.0


# ---------------------------------------------------------------- B. admissibility against exact arithmetic
SHAPES = [(5000, 2048, 1.3, 0), (2049, 2048, 0.5, 8), (6000, 1000, 1.0, 9), (20000, 64, 1.0, 4), (128256, 2048, 0.7, 1)]
# (6000, 1000): a chunk size that is no power of two, 4 tokens per thread with the threads from 250 on empty
HOST_SHAPES = SHAPES[:3]
MAX_AMBIGUOUS = 0.25


@functools.lru_cache(maxsize=None)
def _logits(n, seed):
    x = (np.random.default_rng(seed).standard_normal(n) * 3).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _topk_oracle(n, chunk, temp, seed):
    from oracle import oracle as O
    O.build()
    return O.topk_large_packed(_logits(n, seed), 1, float(np.float32(1.0 / temp)), chunk)


def admissible(x, inv_t, us, tokens, nblocks):
    """asserts the admissibility of every (u, token) of rows that share the logits `x`; returns (exact tokens, mask of the unambiguous rows).
    eps = (nblocks + 32) * 2^-23: nblocks sequential adds of chunk masses + at most 16 thread-local and 8 scan adds + expf and the rescale, each <= 2^-24 of a partial
    sum <= 1; doubled."""
    cdf, logp = exact_cdf(x, inv_t)
    eps = (nblocks + 32) * 2.0 ** -23
    us = np.asarray(us, dtype=np.float64)
    t = tokens.astype(np.int64)
    assert np.all(tokens == t) and np.all((t >= 0) & (t < x.size)), "token ids must be integers inside the row"
    lo = np.where(t > 0, cdf[np.maximum(t - 1, 0)], 0.0)
    ok = (lo - eps <= us) & (us < cdf[t] + eps)
    assert ok.all(), f"{(~ok).sum()} rows outside the exact interval +- eps, e.g. row {np.nonzero(~ok)[0][0]}"
    te = np.minimum(np.searchsorted(cdf, us, side="right"), x.size - 1)
    lo_e = np.where(te > 0, cdf[np.maximum(te - 1, 0)], 0.0)
    clear = (us - lo_e > eps) & (cdf[te] - us > eps)
    assert np.array_equal(t[clear], te[clear]), f"{(t[clear] != te[clear]).sum()} unambiguous rows drew another token than exact arithmetic"
    assert np.all(np.diff(t) >= 0), "tokens must not decrease with u"
    return te, clear, logp


def check_admissible(be, n, chunk, temp, seed):
    x = _logits(n, seed)
    rows = 512 if n > 100000 else 256
    inv_t = np.float32(1.0 / temp)
    us = ((np.arange(rows) + 0.5) / rows).astype(np.float32)
    nb = (n + chunk - 1) // chunk
    pk, bv, bs = run_cat(be, np.broadcast_to(x, (rows, n)), inv_t, us, chunk)
    te, clear, logp = admissible(x, inv_t, us, pk[:, 0], nb)
    print(f"n={n} chunk={chunk}: ambiguous {(~clear).sum()}/{rows}, tokens off the exact one {(pk[:, 0] != te).sum()}")
    assert (~clear).mean() <= MAX_AMBIGUOUS, f"{(~clear).sum()} of {rows} rows ambiguous: the check would hide a failure"
    want_lp = logp[pk[:, 0].astype(np.int64)]
    err = np.abs(pk[:, 1] - want_lp) / (1 + np.abs(want_lp))
    print(f"  logprob: worst error {err.max():.2e} of (1 + |exact|)")
    assert err.max() <= 2e-6
    # the workspace: every row wrote the same chunk maxima, bit for bit, and the normaliser pieces that topk_large_* writes for this row
    pad = np.full(nb * chunk, NINF, np.float32)
    pad[:n] = x
    maxima = pad.reshape(nb, chunk).max(axis=1)
    assert np.array_equal(bv.view(np.uint32), np.broadcast_to(maxima, (rows, nb)).view(np.uint32))
    assert np.array_equal(bs.view(np.uint32), np.broadcast_to(bs[0], (rows, nb)).view(np.uint32))
    ref = _topk_oracle(n, chunk, temp, seed)
    np.testing.assert_allclose(bs[0], ref["block_sums"], rtol=2e-6)
    # denom as the logprob implies it: log denom = x[t] * invT - gmax - logprob.  The oracle's denom is within 2e-6 relative of the exact one (the bound of
    # tests/test_sampling.py), the logprob within 2e-6 (1 + |exact|) by the assertion above: the two may differ by the sum
    t = pk[:, 0].astype(np.int64)
    gmax = np.float64(np.float32(x.max() * inv_t))
    implied = x[t].astype(np.float64) * np.float64(inv_t) - gmax - pk[:, 1].astype(np.float64)
    want = np.log(np.float64(ref["packed"][2])) + (np.float64(ref["packed"][3]) - gmax)
    assert np.abs(implied - want).max() <= 2e-6 * (1 + np.abs(want_lp).max()) + 2e-6, np.abs(implied - want).max()


def check_many_chunks(be, rows):
    """Device only (4500 workgroups per row take a minute on host fibers; checked there once).  More chunks than stage 2 keeps running sums for in LDS (4096): chunks of ONE token, the mass on three tokens past chunk 4096 and on one before it -- the
    walk has to leave the staged part.  The boundaries are few, so nearly every row is unambiguous and must equal the exact token."""
    n = 4500
    x = _row(n, -30.0, i100=1.0, i4200=2.0, i4300=3.0, i4400=1.0)
    us = ((np.arange(rows) + 0.5) / rows).astype(np.float32)
    pk, bv, bs = run_cat(be, np.broadcast_to(x, (rows, n)), 1.0, us, 1)
    te, clear, logp = admissible(x, 1.0, us, pk[:, 0], n)
    assert clear.mean() >= 0.75 and set(pk[:, 0].astype(int)) >= {100, 4200, 4300, 4400}, pk[:, 0]
    t = pk[:, 0].astype(np.int64)
    assert np.abs(pk[:, 1] - logp[t]).max() <= 2e-6 * (1 + np.abs(logp[t]).max())
    assert np.array_equal(bv[0].view(np.uint32), x.view(np.uint32)) and np.all(bs == 1.0)


# ---------------------------------------------------------------- D. stage 1 is ONE piece of arithmetic behind three entry points
STAGE1_SHAPES = [(300, 64), (700, 256), (4101, 4096)]
# (300, 64): five chunks, a ragged last one, most threads idle; (700, 256): a chunk exactly one thread stride wide; (4101, 4096): all 16 registers per thread, then a
# 5-token tail chunk


def check_stage1_shared(be, n, chunk):
    """top-k (k = 1), the categorical draw and the nucleus draw leave the SAME chunk sums and chunk maxima for the same logits and temperatures, bit for bit: the
    normaliser of all three is one computation.  No NaN (the two families report a NaN chunk's maximum differently by contract) and no chunk maximum of +-0 (the
    key route and fmaxf may legitimately differ in its sign)."""
    rows, nb = 2, (n + chunk - 1) // chunk
    x = (np.random.default_rng(n).standard_normal((rows, n)) * 3).astype(np.float32)
    for r in range(rows):  # one chunk of nothing but -inf per row, another chunk in each
        b = (1 + r) % nb
        x[r, b * chunk:(b + 1) * chunk] = NINF
    pad = np.full((rows, nb * chunk), NINF, np.float32)
    pad[:, :n] = x
    assert not np.any(pad.reshape(rows, nb, chunk).max(axis=2) == 0)
    inv_t = (1.0 / np.array([0.7, 1.3])).astype(np.float32)
    us = np.array([0.25, 0.75], np.float32)
    ws = lambda per_row: be.buf(np.full(rows * per_row, 7.0, np.float32))
    xb, tb, ub = be.buf(x), be.buf(inv_t), be.buf(us)
    k_bv, k_bi, k_bm, k_bs, k_pk = ws(nb), be.buf(np.zeros(rows * nb, np.uint32)), ws(nb), ws(nb), ws(4)
    be.sym("topk_large_f32_packed_batched", [VP] * 7 + [I] * 5 + [LL])(xb.ptr, tb.ptr, k_bv.ptr, k_bi.ptr, k_bm.ptr, k_bs.ptr, k_pk.ptr, rows, n, 1, chunk, nb,
                                                                       be.stream or 0)
    c_bv, c_bs, c_pk = ws(nb), ws(nb), ws(2)
    be.sym("categorical_large_f32_packed_batched", [VP] * 6 + [I] * 4 + [LL])(xb.ptr, tb.ptr, ub.ptr, c_bv.ptr, c_bs.ptr, c_pk.ptr, rows, n, chunk, nb, be.stream or 0)
    n_bv, n_bs, n_pk = ws(nb), ws(nb), ws(4)
    pb, mb = be.buf(np.full(rows, 0.9, np.float32)), be.buf(np.zeros(rows, np.float32))
    be.sym("mrs_nucleus_large_f32_packed_batched", [VP] * 8 + [I] * 4 + [LL])(xb.ptr, tb.ptr, ub.ptr, pb.ptr, mb.ptr, n_bv.ptr, n_bs.ptr, n_pk.ptr, rows, n, chunk, nb,
                                                                              be.stream or 0)
    bits = lambda b: np.ascontiguousarray(b.numpy(), dtype=np.float32).reshape(rows, nb).view(np.uint32)
    assert np.isfinite(c_pk.numpy()).all() and np.isfinite(n_pk.numpy()).all()  # every launch ran
    assert np.array_equal(bits(k_bs), bits(c_bs)) and np.array_equal(bits(c_bs), bits(n_bs))
    scaled = (c_bv.numpy().reshape(rows, nb).astype(np.float32) * inv_t[:, None]).astype(np.float32)
    assert np.array_equal(scaled.view(np.uint32), bits(k_bm))
    assert np.array_equal(bits(n_bv), bits(c_bv))


# ---------------------------------------------------------------- the two backends
@pytest.fixture(scope="module")
def host():
    from tests.abi_backends import HostBackend
    return HostBackend()


@pytest.mark.parametrize("n,chunk", STAGE1_SHAPES, ids=[f"n{s[0]}c{s[1]}" for s in STAGE1_SHAPES])
def test_stage1_shared_host_emulation(host, n, chunk):
    check_stage1_shared(host, n, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunk", STAGE1_SHAPES, ids=[f"n{s[0]}c{s[1]}" for s in STAGE1_SHAPES])
def test_stage1_shared_gpu(dev, n, chunk):
    from tests.abi_backends import GpuBackend
    check_stage1_shared(GpuBackend(dev), n, chunk)


def test_exact_cases_host_emulation(host):
    check_exact_cases(host)


def test_invalid_rows_host_emulation(host):
    check_invalid_rows(host)


def test_launcher_refuses_host_emulation(host):
    check_launcher_refuses(host)


@pytest.mark.parametrize("n,chunk,temp,seed", HOST_SHAPES, ids=[f"n{s[0]}c{s[1]}" for s in HOST_SHAPES])
def test_admissible_host_emulation(host, n, chunk, temp, seed):
    check_admissible(host, n, chunk, temp, seed)


@pytest.mark.gpu
def test_many_chunks_gpu(dev):
    from tests.abi_backends import GpuBackend
    check_many_chunks(GpuBackend(dev), 64)


@pytest.mark.gpu
def test_exact_cases_gpu(dev):
    from tests.abi_backends import GpuBackend
    check_exact_cases(GpuBackend(dev))


@pytest.mark.gpu
def test_invalid_rows_gpu(dev):
    from tests.abi_backends import GpuBackend
    check_invalid_rows(GpuBackend(dev))


@pytest.mark.gpu
def test_launcher_refuses_gpu(dev):
    from tests.abi_backends import GpuBackend
    check_launcher_refuses(GpuBackend(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunk,temp,seed", SHAPES, ids=[f"n{s[0]}c{s[1]}" for s in SHAPES])
def test_admissible_gpu(dev, n, chunk, temp, seed):
    from tests.abi_backends import GpuBackend
    check_admissible(GpuBackend(dev), n, chunk, temp, seed)


# ---------------------------------------------------------------- the host statement of the rule, and the helpers around it (no device)
def test_categorical_host_states_the_rule():
    from mistralrs_amd import sampler
    z = np.array([NINF, 0, NINF, 0, NINF], np.float32)
    assert [sampler.categorical_host(z, 1.0, u)[0] for u in (0.0, 0.25, 0.5, 0.75, U_TOP)] == [1, 1, 3, 3, 3]
    tok, lp = sampler.categorical_host(np.zeros(2048, np.float32), 1.0, U_TOP)
    assert tok == 2047 and abs(lp + np.log(2048.0)) < 1e-6
    assert sampler.categorical_host(_row(2051, -20.0, i2049=4.0), 0.5, 0.5)[0] == 2049
    x = _logits(5000, 0)
    us = ((np.arange(256) + 0.5) / 256).astype(np.float32)
    inv_t = np.float32(1.0 / 1.3)
    got = [sampler.categorical_host(x, inv_t, u) for u in us]
    te, clear, logp = admissible(x, inv_t, us, np.array([g[0] for g in got], np.float32), 5000)  # one chunk, 5000 sequential adds: the same eps formula
    np.testing.assert_allclose([g[1] for g in got], logp[[g[0] for g in got]], rtol=2e-6, atol=2e-6)
    bad = [(np.append(x, np.float32(np.nan)), 1.0, 0.5), (np.append(x, np.float32(np.inf)), 1.0, 0.5), (np.full(9, NINF), 1.0, 0.5), (x, 0.0, 0.5), (x, 1.0, 1.0),
           (x, 1.0, -0.1), (x, np.inf, 0.5)]
    for row, it, u in bad:
        with pytest.raises(ValueError, match="invalid batched CUDA categorical output"):
            sampler.categorical_host(row, it, u)


def test_uniform_for_and_categorical_token():
    from mistralrs_amd import sampler
    us = [sampler.uniform_for(5, i) for i in range(64)]
    assert all(isinstance(u, np.float32) and 0 <= u < 1 for u in us) and len(set(us)) == 64
    assert us[::-1] == [sampler.uniform_for(5, i) for i in reversed(range(64))]  # a function of (seed, index), not of the call order
    assert sampler.uniform_for(6, 0) != us[0]
    assert sampler.categorical_token(np.array([17.0, -0.5], np.float32)) == (17, -0.5)
    for pair in ([np.nan, np.nan], [-1.0, -0.5], [1.5, -0.5], [3.0, np.nan], [3.0, -np.inf], [np.inf, 0.0]):
        with pytest.raises(ValueError, match="invalid batched CUDA categorical output"):
            sampler.categorical_token(np.array(pair, np.float32))


# ---------------------------------------------------------------- C. the Python surface on the device
@pytest.mark.gpu
def test_categorical_class_gpu(dev):
    import torch
    from mistralrs_amd import sampler
    n = 128256
    x = _logits(n, 1)
    cat = sampler.Categorical(n, dev, max_rows=2)
    assert cat.nblocks == 63
    for u in (0.013, 0.37, 0.5, 0.93):
        tok, lp = sampler.categorical_token(cat(torch.from_numpy(x.copy()).to(dev), 0.7, [u]).cpu().numpy()[0])
        te, clear, logp = admissible(x, np.float32(1.0 / 0.7), [np.float32(u)], np.array([tok], np.float32), 63)
        if clear[0]:
            assert tok == sampler.categorical_host(x, np.float32(1.0 / 0.7), np.float32(u))[0] == te[0]
        assert abs(lp - logp[tok]) <= 2e-6 * (1 + abs(logp[tok]))
    y = x[::-1].copy()
    two = torch.from_numpy(np.stack([x, y])).to(dev)
    pk = cat(two, [0.7, 1.5], [0.25, 0.75]).cpu().numpy()
    for row, temp, u, p in ((x, 0.7, 0.25, pk[0]), (y, 1.5, 0.75, pk[1])):
        inv_t = np.float32(1.0 / temp)
        tok, lp = sampler.categorical_token(p)
        te, clear, logp = admissible(row, inv_t, [np.float32(u)], np.array([tok], np.float32), 63)
        if clear[0]:
            assert tok == sampler.categorical_host(row, inv_t, np.float32(u))[0]
    with pytest.raises(ValueError):
        cat(two, 0.0, [0.5, 0.5])
    with pytest.raises(ValueError):
        cat(two, [0.7, np.inf], [0.5, 0.5])
    with pytest.raises(ValueError):
        cat(two, 1.0, [0.5, 1.0])
    with pytest.raises(ValueError):
        cat(two, 1.0, [0.5])
    with pytest.raises(ValueError):
        cat(torch.zeros(3, n, device=dev), 1.0, [0.5] * 3)  # more rows than the workspace
    with pytest.raises(ValueError):
        cat(two.double(), 1.0, [0.5, 0.5])
    with pytest.raises(ValueError):
        sampler.Categorical(2 ** 24 + 1, dev)
    with pytest.raises(ValueError):
        sampler.Categorical(0, dev)
    with pytest.raises(ValueError):
        sampler.Categorical(n, dev, max_rows=65536)


@pytest.mark.gpu
def test_generate_without_top_k_on_the_runner(oracle, dev):
    """top_k = 0: a fixed seed reproduces the run; every token is what `categorical_host` draws from that step's logits at uniform_for(seed, i), or is admissible
    where the uniform sits within f32 rounding of a boundary; probabilities are probabilities; top_p without top_k is refused"""
    from tests.test_dec_model import Q4KM, _mk
    from mistralrs_amd import sampler
    cfg, w, m, cos, sin = _mk(oracle, dev, Q4KM(oracle), "bf16")
    prompt = [(1000 + 7 * i) % cfg.vocab_size for i in range(12)]
    a = sampler.generate(m, prompt, 8, top_k=0, temperature=1.5, seed=5)
    b = sampler.generate(m, prompt, 8, top_k=None, temperature=1.5, seed=5)
    assert a == b and len(a[0]) == 8
    assert all(0 <= t < cfg.vocab_size for t in a[0]) and all(0 < p <= 1 for p in a[1])
    inv_t, nb = np.float32(1.0 / 1.5), (cfg.vocab_size + 2047) // 2048
    lg = m.prefill(prompt, 0)
    for i, (tok, p) in enumerate(zip(*a)):
        x = lg.float().reshape(-1).cpu().numpy()
        u = sampler.uniform_for(5, i)
        te, clear, logp = admissible(x, inv_t, [u], np.array([tok], np.float32), nb)
        if clear[0]:
            assert tok == sampler.categorical_host(x, inv_t, u)[0]
        assert abs(np.log(p) - logp[tok]) <= 2e-6 * (1 + abs(logp[tok])) + 1e-7
        m.set_state([tok], [len(prompt) + i])
        lg = m.forward_logits(1)[0]
    with pytest.raises(ValueError, match="top_k"):
        sampler.generate(m, prompt, 2, top_k=0, top_p=0.9)
    with pytest.raises(ValueError, match="top_k"):
        sampler.generate(m, prompt, 2, top_k=0, min_p=0.1)
