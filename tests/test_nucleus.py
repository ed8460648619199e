"""Device top-p / min-p draw over the whole vocabulary (csrc/sampling.hip, `mrs_nucleus_large_f32_packed_batched`), checked against EXACT arithmetic (float64) as
tests/test_categorical.py does.  Every body takes a backend of tests/abi_backends.py -- the host emulation in the CPU suite, the MI355X under `-m gpu` -- or
`HostRule`, which answers the same launches with `sampler.nucleus_host`.

eps = (nblocks + 32) * 2^-23 is test_categorical's bound and is kept although the kernel needs less: its masses are integers q_i = floor(w_i * 2^39), summed exactly,
so against float64 only expf's rounding (<= 2^-23 relative per weight, hence of any sum of weights) and the truncation (n * 2^-39 absolute, < 2^-22 for n <= 2^17,
against a total >= 1) remain.

min-p follows the rule `w_i > min_p` on the weights relative to the largest (the reference's `max_p * min_p >= p` removes).  On probabilities (0.5, 0.3, 0.15, 0.05)
that rule keeps {0.5, 0.3, 0.15} at min_p = 0.2 and {0.5, 0.3} at min_p = 0.4; {0.5} alone needs min_p >= 0.6.  All three kept sets are checked."""
import ctypes as C
import functools

import numpy as np
import pytest

VP, I, LL = C.c_void_p, C.c_int, C.c_int64
U_TOP = np.float32(1.0 - 2.0 ** -24)
NINF = np.float32(-np.inf)
SYM = "mrs_nucleus_large_f32_packed_batched"


def run_nuc(be, xs, inv_t, us, top_p, min_p, chunk, nblocks=None, rows_arg=None):
    """one batched launch: packed [rows, 4] (prefilled with the sentinel 7)"""
    rows = len(us)
    xs = np.ascontiguousarray(xs, dtype=np.float32).reshape(rows, -1)
    n = xs.shape[1]
    nb = (n + chunk - 1) // chunk if nblocks is None else nblocks
    col = lambda v: be.buf(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (rows,))))
    xb, tb, ub, pb, mb = be.buf(xs), col(inv_t), col(us), col(top_p), col(min_p)
    nbuf = max(rows * nb, 1)
    bv, bs, pk = be.buf(np.full(nbuf, 7.0, np.float32)), be.buf(np.full(nbuf, 7.0, np.float32)), be.buf(np.full(rows * 4, 7.0, np.float32))
    be.sym(SYM, [VP, VP, VP, VP, VP, VP, VP, VP, I, I, I, I, LL])(xb.ptr, tb.ptr, ub.ptr, pb.ptr, mb.ptr, bv.ptr, bs.ptr, pk.ptr, rows if rows_arg is None else rows_arg, n,
                                                                 chunk, nb, be.stream or 0)
    return pk.numpy().reshape(rows, 4)


class HostRule:
    """`sampler.nucleus_host` behind the launcher's interface: bodies 1 to 3 run on it unchanged"""
    name, stream = "nucleus_host", None

    class _Buf:
        def __init__(self, a):
            self.a = np.ascontiguousarray(a).copy()
            self.ptr = self

        def numpy(self):
            return self.a

    def buf(self, a, dtype=None):
        return self._Buf(a)

    def sym(self, name, argtypes, restype=None):
        assert name == SYM
        from mistralrs_amd import sampler

        def launch(x, t, u, p, m, bv, bs, pk, rows, n, chunk, nb, stream):
            xs = x.a.reshape(rows, n)
            for r in range(rows):
                try:
                    pk.a[4 * r: 4 * r + 4] = sampler.nucleus_host(xs[r], t.a[r], u.a[r], p.a[r], m.a[r])
                except ValueError:
                    pk.a[4 * r: 4 * r + 4] = np.nan
        return launch


def exact(x, inv_t):
    """float64 weights relative to the largest, and the log-probabilities, at the f32 inverse temperature the kernel gets"""
    z = x.astype(np.float64) * np.float64(np.float32(inv_t))
    z -= z.max()
    w = np.exp(z)
    return w, z - np.log(w.sum())


# ---------------------------------------------------------------- 1. exact cases
P4 = np.array([0.5, 0.3, 0.15, 0.05])
AT = [3, 100, 2048, 2050]  # two of them in the ragged second chunk at chunk_size 2048


def four_row():
    x = np.full(2051, NINF, np.float32)
    x[AT] = np.log(P4).astype(np.float32)
    return x


def kept_tokens(be, x, top_p, min_p, chunk=2048, rows=64):
    us = np.r_[(np.arange(rows - 1) / (rows - 1)).astype(np.float32), U_TOP]
    pk = run_nuc(be, np.broadcast_to(x, (rows, x.size)), 1.0, us, top_p, min_p, chunk)
    assert np.all(np.diff(pk[:, 0]) >= 0)
    return sorted(set(pk[:, 0].astype(int))), pk


def check_exact_cases(be):
    x = four_row()
    logp = exact(x, 1.0)[1]
    toks, pk = kept_tokens(be, x, 0.7, 0.0)
    assert toks == AT[:2], toks
    assert np.all(pk[:, 2] == np.float32(np.log(0.3))) and np.allclose(pk[:, 3], 0.8, rtol=0, atol=1e-6), pk[0]
    np.testing.assert_allclose(pk[:, 1], logp[pk[:, 0].astype(int)], rtol=2e-6, atol=2e-6)  # under the FULL softmax: log 0.5 / log 0.3, not / 0.8
    us = np.array([0.0, 0.3, 0.62, 0.63, 0.9, U_TOP], np.float32)  # the switch is at 0.5 / 0.8 = 0.625
    pk = run_nuc(be, np.broadcast_to(x, (6, x.size)), 1.0, us, 0.7, 0.0, 2048)
    assert pk[:, 0].tolist() == [3, 3, 3, 100, 100, 100], pk[:, 0]
    for min_p, want, share in ((0.2, AT[:3], 0.95), (0.4, AT[:2], 0.8), (0.8, AT[:1], 0.5)):
        toks, pk = kept_tokens(be, x, 1.0, min_p)
        assert toks == want, (min_p, toks)
        assert np.all(pk[:, 2] == NINF) and np.allclose(pk[:, 3], share, rtol=0, atol=1e-6), (min_p, pk[0])
    toks, pk = kept_tokens(be, x, 0.95, 0.4)  # top-p keeps at least three, min-p the first two: the intersection
    assert toks == AT[:2] and np.allclose(pk[:, 3], 0.8, rtol=0, atol=1e-6), (toks, pk[0])
    toks, pk = kept_tokens(be, x, 0.95, 0.2)
    assert toks == AT[:3] and np.allclose(pk[:, 3], 0.95, rtol=0, atol=1e-6), (toks, pk[0])
    toks, pk = kept_tokens(be, x, 0.4, 0.2, chunk=1000)  # another chunking, the top token alone
    assert toks == AT[:1] and np.all(pk[:, 2] == np.float32(np.log(0.5))), (toks, pk[0])
    # the tie rule: four equal logits, top_p = 0.5 keeps ALL of them
    toks, pk = kept_tokens(be, np.zeros(4, np.float32), 0.5, 0.0, chunk=2)
    assert toks == [0, 1, 2, 3] and np.all(pk[:, 2] == 0.0) and np.all(pk[:, 3] == 1.0), (toks, pk[0])
    np.testing.assert_allclose(pk[:, 1], np.log(0.25), rtol=2e-6)
    # a cut value of 0, 1, 1.5 or NaN is inactive: x* = -inf, share 1, the token is categorical's
    from tests.test_categorical import _logits, admissible
    y = _logits(2049, 8)
    us = ((np.arange(8) + 0.5) / 8).astype(np.float32)
    for v in (0.0, 1.0, 1.5, np.nan):
        pk = run_nuc(be, np.broadcast_to(y, (8, y.size)), 0.5, us, v, v, 2048)
        assert np.all(pk[:, 2] == NINF) and np.all(pk[:, 3] == 1.0), (v, pk)
        te, clear, lp = admissible(y, 0.5, us, pk[:, 0], 2)
        np.testing.assert_allclose(pk[:, 1], lp[pk[:, 0].astype(int)], rtol=2e-6, atol=2e-6)
    # a zero-weight token is never returned; one column
    z = np.array([NINF, 0, NINF, 0, NINF], np.float32)
    pk = run_nuc(be, np.tile(z, (5, 1)), 1.0, [0.0, 0.25, 0.5, 0.75, U_TOP], 0.9, 0.0, 2)
    assert pk[:, 0].tolist() == [1, 1, 3, 3, 3], pk
    pk = run_nuc(be, np.array([[-3.5]], np.float32), 0.7, [0.99], 0.9, 0.1, 2048)
    assert pk[0].tolist() == [0.0, 0.0, -3.5, 1.0], pk


# ---------------------------------------------------------------- 2. the threshold against float64
THRESHOLD_SHAPES = [(5, 2, 11), (2051, 2048, 12), (4099, 1000, 13), (6000, 4096, 14)]
BIG = (128256, 2048, 15)
TEMPS, TOP_PS = (0.7, 2.5), (0.1, 0.9, 0.99)


@functools.lru_cache(maxsize=None)
def tied_logits(n, seed):
    """Gaussian logits, every eighth one a copy of another (planted ties)"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 3).astype(np.float32)
    dst = g.permutation(n)[: max(1, n // 8)]
    x[dst] = x[g.integers(0, n, dst.size)]
    x.setflags(write=False)
    return x


def check_threshold(be, n, chunk, seed):
    x = tied_logits(n, seed)
    nb = (n + chunk - 1) // chunk
    eps = (nb + 32) * 2.0 ** -23
    cases = [(t, p) for t in TEMPS for p in TOP_PS]
    inv_ts = [np.float32(1.0 / t) for t, _ in cases]
    pk = run_nuc(be, np.broadcast_to(x, (len(cases), n)), inv_ts, [0.5] * len(cases), [p for _, p in cases], 0.0, chunk)
    for (t, p), inv_t, row in zip(cases, inv_ts, pk):
        w, _ = exact(x, inv_t)
        xs = row[2]
        assert np.any(x == xs), f"x* = {xs} does not occur in the row"
        gt, ge, tp = w[x > xs].sum() / w.sum(), w[x >= xs].sum() / w.sum(), np.float64(np.float32(p))
        print(f"n={n} T={t} top_p={p}: x*={xs:.6g} S_gt={gt:.9f} S_ge={ge:.9f} share={row[3]:.9f} kept={int((x >= xs).sum())}")
        assert gt < tp * (1 + eps) and ge >= tp * (1 - eps), (n, t, p, gt, ge)
        assert abs(np.float64(row[3]) - ge) <= eps, (row[3], ge)


# ---------------------------------------------------------------- 3. the draw against float64, given the reported x*
# flat rows that keep thousands of tokens put ~2 eps / (1 / kept) of the uniforms next to a boundary: the cases keep at most ~1000 tokens
DRAW_CASES = [(5, 2, 11, 0.7, 0.9, 0.0), (2051, 2048, 12, 2.5, 0.9, 0.05), (4099, 1000, 13, 0.7, 0.99, 0.0), (6000, 4096, 14, 2.5, 0.1, 0.0), (6000, 4096, 14, 0.7, 1.0, 0.02)]
MAX_AMBIGUOUS = 0.02


def check_draw(be, n, chunk, seed, temp, top_p, min_p, rows=257):
    x = tied_logits(n, seed)
    inv_t = np.float32(1.0 / temp)
    nb = (n + chunk - 1) // chunk
    eps = (nb + 32) * 2.0 ** -23
    us = np.r_[np.float32(0), ((np.arange(rows - 2) + 0.5) / (rows - 2)).astype(np.float32), U_TOP]
    pk = run_nuc(be, np.broadcast_to(x, (rows, n)), inv_t, us, top_p, min_p, chunk)
    assert np.array_equal(pk[:, 2:].view(np.uint32), np.broadcast_to(pk[0, 2:], (rows, 2)).view(np.uint32))  # x* and the share do not depend on u
    xs = pk[0, 2]
    w, logp = exact(x, inv_t)
    w32 = np.exp((x * inv_t - np.float32(x.max() * inv_t)).astype(np.float32), dtype=np.float32)
    keep = (x >= xs) & ((w32 > np.float32(min_p)) if 0 < min_p < 1 else True)
    # a weight within f32 rounding of min_p may fall on either side on the device (its expf is not numpy's): such tokens are allowed, not required
    edge = np.abs(w32 - np.float32(min_p)) <= 4 * 2.0 ** -24 if 0 < min_p < 1 else np.zeros(n, bool)
    assert not edge.any(), "choose another seed: a weight sits on the min-p boundary"
    t = pk[:, 0].astype(np.int64)
    assert np.all(pk[:, 0] == t) and np.all((t >= 0) & (t < n)) and keep[t].all(), "a token outside the kept set"
    cdf = np.cumsum(np.where(keep, w, 0.0))
    cdf /= cdf[-1]
    u64 = us.astype(np.float64)
    lo = np.where(t > 0, cdf[np.maximum(t - 1, 0)], 0.0)
    ok = (lo - eps <= u64) & (u64 < cdf[t] + eps)
    assert ok.all(), f"{(~ok).sum()} rows outside the exact interval +- eps"
    te = np.minimum(np.searchsorted(cdf, u64, side="right"), n - 1)
    lo_e = np.where(te > 0, cdf[np.maximum(te - 1, 0)], 0.0)
    clear = (u64 - lo_e > eps) & (cdf[te] - u64 > eps)
    print(f"n={n} chunk={chunk} T={temp} top_p={top_p} min_p={min_p}: kept {int(keep.sum())}, ambiguous {(~clear).sum()}/{rows}, off the exact token {(t != te).sum()}")
    assert np.array_equal(t[clear], te[clear]), f"{(t[clear] != te[clear]).sum()} unambiguous rows drew another token than exact arithmetic"
    assert np.all(np.diff(t) >= 0), "tokens must not decrease with u"
    assert (~clear).mean() <= MAX_AMBIGUOUS, f"{(~clear).sum()} of {rows} rows ambiguous: the check would hide a failure"
    err = np.abs(pk[:, 1] - logp[t]) / (1 + np.abs(logp[t]))
    assert err.max() <= 2e-6, err.max()


# ---------------------------------------------------------------- 4. determinism and isolation
def check_isolation(be):
    n, chunk = 2051, 2048
    x, other, bad = tied_logits(n, 12), tied_logits(n, 21), tied_logits(n, 22).copy()
    bad[2050] = np.nan
    par = dict(inv_t=np.float32(1 / 0.7), u=0.37, top_p=0.9, min_p=0.01)
    alone = run_nuc(be, x[None], par["inv_t"], [par["u"]], par["top_p"], par["min_p"], chunk)
    assert np.isfinite(alone).all()
    first = run_nuc(be, np.stack([x, other, bad]), [par["inv_t"], 1.0, 0.5], [par["u"], 0.9, 0.1], [par["top_p"], 0.5, 0.9], [par["min_p"], 0.0, 0.2], chunk)
    last = run_nuc(be, np.stack([bad, other, x]), [2.0, 0.3, par["inv_t"]], [0.5, 0.2, par["u"]], [0.3, 0.99, par["top_p"]], [0.0, 0.1, par["min_p"]], chunk)
    again = run_nuc(be, np.stack([bad, other, x]), [2.0, 0.3, par["inv_t"]], [0.5, 0.2, par["u"]], [0.3, 0.99, par["top_p"]], [0.0, 0.1, par["min_p"]], chunk)
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32).tolist()
    assert bits(first[0]) == bits(alone[0]) == bits(last[2]), (alone, first, last)
    assert bits(last) == bits(again)
    assert np.isnan(first[2]).all() and np.isnan(last[0]).all() and np.isfinite(first[1]).all() and np.isfinite(last[1]).all()


def check_invalid_rows(be):
    n = 2051
    good = four_row()
    with_inf, all_ninf = good.copy(), np.full(n, NINF, np.float32)
    with_inf[7] = np.inf
    rows = [good, with_inf, all_ninf, good, good, good, good, good, good]
    inv_t = [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, -1.0, np.inf, 1.0]
    us = [0.2, 0.2, 0.2, 0.2, 1.0, -0.1, 0.2, 0.2, np.nan]
    pk = run_nuc(be, np.stack(rows), inv_t, us, 0.7, 0.0, 2048)
    assert pk[0].tolist()[0] == 3.0 and np.isfinite(pk[0]).all()
    assert np.isnan(pk[1:]).all(), pk


# ---------------------------------------------------------------- 5. launcher refusals
def check_launcher_refuses(be):
    """shapes outside the launcher return without launching: the output keeps the sentinel"""
    x = np.zeros((1, 100), np.float32)
    for chunk, nb in ((0, 1), (4097, 1), (10, 9)):
        pk = run_nuc(be, x, 1.0, [0.5], 0.9, 0.0, chunk, nblocks=nb)
        assert pk[0].tolist() == [7.0] * 4, (chunk, nb, pk)
    assert run_nuc(be, x, 1.0, [0.5], 0.9, 0.0, 100, rows_arg=0)[0].tolist() == [7.0] * 4
    pk = run_nuc(be, x, 1.0, [0.5], 0.9, 0.0, 4096)
    assert pk[0, 0] == 50.0 and abs(pk[0, 1] + np.log(100.0)) < 1e-5 and pk[0, 2] == 0.0 and pk[0, 3] == 1.0, pk


# ---------------------------------------------------------------- the backends
@pytest.fixture(scope="module")
def host():
    from tests.abi_backends import HostBackend
    return HostBackend()


@pytest.fixture(scope="module")
def gpu(dev):
    from tests.abi_backends import GpuBackend
    return GpuBackend(dev)


def test_exact_cases_host_emulation(host):
    check_exact_cases(host)


def test_invalid_rows_and_isolation_host_emulation(host):
    check_invalid_rows(host)
    check_isolation(host)


def test_launcher_refuses_host_emulation(host):
    check_launcher_refuses(host)


@pytest.mark.parametrize("n,chunk,seed", THRESHOLD_SHAPES, ids=[f"n{s[0]}c{s[1]}" for s in THRESHOLD_SHAPES])
def test_threshold_host_emulation(host, n, chunk, seed):
    check_threshold(host, n, chunk, seed)


@pytest.mark.parametrize("case", DRAW_CASES[:2], ids=[f"n{c[0]}c{c[1]}" for c in DRAW_CASES[:2]])
def test_draw_host_emulation(host, case):
    check_draw(host, *case)


def test_nucleus_host_states_the_rule():
    be = HostRule()
    check_exact_cases(be)
    check_invalid_rows(be)
    check_isolation(be)
    for n, chunk, seed in THRESHOLD_SHAPES + [BIG]:
        check_threshold(be, n, chunk, seed)
    for case in DRAW_CASES:
        check_draw(be, *case)


def test_nucleus_token_and_cut_active():
    from mistralrs_amd import sampler
    assert sampler.nucleus_token(np.array([17.0, -0.5, 1.25, 0.9], np.float32)) == (17, -0.5)
    assert sampler.nucleus_token(np.array([17.0, -0.5, -np.inf, 1.0], np.float32)) == (17, -0.5)
    for row in ([np.nan] * 4, [-1.0, -0.5, 0, 1], [1.5, -0.5, 0, 1], [3.0, np.nan, 0, 1], [3.0, -np.inf, 0, 1], [np.inf, 0.0, 0, 1], [3.0, -0.5, np.nan, 1]):
        with pytest.raises(ValueError, match="invalid batched nucleus output"):
            sampler.nucleus_token(np.array(row, np.float32))
    assert [sampler.cut_active(v) for v in (None, 0.0, 1.0, 1.5, float("nan"), -0.1, 0.9, 1e-6)] == [False] * 6 + [True] * 2
    with pytest.raises(ValueError, match="invalid batched nucleus output"):
        sampler.nucleus_host(np.array([0.0, np.nan], np.float32), 1.0, 0.5, 0.9)


@pytest.mark.gpu
def test_exact_cases_gpu(gpu):
    check_exact_cases(gpu)


@pytest.mark.gpu
def test_invalid_rows_and_isolation_gpu(gpu):
    check_invalid_rows(gpu)
    check_isolation(gpu)


@pytest.mark.gpu
def test_launcher_refuses_gpu(gpu):
    check_launcher_refuses(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunk,seed", THRESHOLD_SHAPES + [BIG], ids=[f"n{s[0]}c{s[1]}" for s in THRESHOLD_SHAPES + [BIG]])
def test_threshold_gpu(gpu, n, chunk, seed):
    check_threshold(gpu, n, chunk, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DRAW_CASES, ids=[f"n{c[0]}c{c[1]}p{c[4]}" for c in DRAW_CASES])
def test_draw_gpu(gpu, case):
    check_draw(gpu, *case)


@pytest.mark.gpu
def test_nucleus_class_gpu(dev):
    import torch
    from mistralrs_amd import sampler
    n = 6000
    x, y = tied_logits(n, 14), tied_logits(n, 14)[::-1].copy()
    nuc = sampler.Nucleus(n, dev, max_rows=2)
    assert nuc.nblocks == 3
    two = torch.from_numpy(np.stack([x, y])).to(dev)
    pk = nuc(two, [0.7, 1.5], [0.25, 0.75], [0.9, 1.0], [0.0, 0.05]).cpu().numpy()
    for row, temp, u, tp, mp, p in ((x, 0.7, 0.25, 0.9, 0.0, pk[0]), (y, 1.5, 0.75, 1.0, 0.05, pk[1])):
        tok, lp = sampler.nucleus_token(p)
        want = sampler.nucleus_host(row, np.float32(1.0 / temp), np.float32(u), tp, mp)
        _, logp = exact(row, np.float32(1.0 / temp))
        assert abs(lp - logp[tok]) <= 2e-6 * (1 + abs(logp[tok]))
        assert p[2] == np.float32(want[2]) and abs(p[3] - want[3]) <= 35 * 2.0 ** -23, (p, want)
    one = sampler.nucleus_token(nuc(two[0], 0.7, [0.25], 0.9).cpu().numpy()[0])
    assert one == sampler.nucleus_token(pk[0])
    for args in ((two, 0.0, [0.5, 0.5]), (two, [0.7, np.inf], [0.5, 0.5]), (two, 1.0, [0.5, 1.0]), (two, 1.0, [0.5]), (torch.zeros(3, n, device=dev), 1.0, [0.5] * 3),
                 (two.double(), 1.0, [0.5, 0.5])):
        with pytest.raises(ValueError):
            nuc(*args, 0.9)
    for v, kw in ((2 ** 24 + 1, {}), (0, {}), (n, dict(max_rows=65536))):
        with pytest.raises(ValueError):
            sampler.Nucleus(v, dev, **kw)
