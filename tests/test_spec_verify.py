"""The speculative verifier (csrc/sampling.hip `mrs_spec_verify_f32_batched`) and the state advance after a round (csrc/ext_decode.hip `mrs_spec_advance`).
Greedy rounds are checked exactly (winners are `mrs_sample_greedy_advance`'s), the stochastic rule exactly where the arithmetic leaves no choice, against float64 with the
definitions of tests/test_categorical.py part B elsewhere, and by its law: over a grid of uniforms the emitted tokens are distributed as the target.
Every body takes a backend of tests/abi_backends.py: the host emulation in the CPU suite, the MI355X under `-m gpu`."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

from tests.test_categorical import MAX_AMBIGUOUS, NINF, U_TOP, run_cat

VP, I, LL, SZ = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEDY, TEMP = 0, 1
KEEP = 7  # what the outputs hold before a launch: a refused launch leaves it


def run_verify(be, target, draft_ids, seq_rows, modes, inv_t, us, chunk, draft=None, nblocks=None, ws_cut=0, nseq=None, total_rows=None):
    """one launch group: (n_accepted [nseq], out_tokens [nseq, 8])"""
    target = np.ascontiguousarray(target, dtype=np.float32)
    rows, n = target.shape
    seqs = len(seq_rows) - 1
    nb = (n + chunk - 1) // chunk if nblocks is None else nblocks
    modes = np.broadcast_to(np.asarray(modes, dtype=np.int32), (seqs,))
    inv_t = np.broadcast_to(np.asarray(inv_t, dtype=np.float32), (seqs,))
    us = np.zeros((rows, 2), np.float32) if us is None else np.asarray(us, dtype=np.float32).reshape(rows, 2)
    need = be.sym("mrs_spec_verify_workspace_bytes", [I, I, I], SZ)(rows, max(seqs, 1), max(nb, 1))
    assert need > 0
    tb, ib, sb = be.buf(target), be.buf(np.asarray(draft_ids, dtype=np.int32)), be.buf(np.asarray(seq_rows, dtype=np.int32))
    mb, vb, ub = be.buf(np.ascontiguousarray(modes)), be.buf(np.ascontiguousarray(inv_t)), be.buf(np.ascontiguousarray(us))
    db = be.buf(np.ascontiguousarray(draft, dtype=np.float32)) if draft is not None else None
    ws = be.buf(np.zeros(need // 8 + 1, np.int64))
    na, ot = be.buf(np.full(max(seqs, 1), KEEP, np.int32)), be.buf(np.full(max(seqs, 1) * 8, KEEP, np.int32))
    be.sym("mrs_spec_verify_f32_batched", [VP] * 8 + [SZ, VP, VP, I, I, I, I, I, LL])(
        tb.ptr, db.ptr if db is not None else None, ib.ptr, sb.ptr, mb.ptr, vb.ptr, ub.ptr, ws.ptr, need - ws_cut, na.ptr, ot.ptr,
        seqs if nseq is None else nseq, rows if total_rows is None else total_rows, n, chunk, nb, be.stream or 0)
    return na.numpy().astype(np.int64).reshape(-1), ot.numpy().astype(np.int64).reshape(-1, 8)


def greedy_advance_winners(be, rows):
    """the token `mrs_sample_greedy_advance` picks on each row (<= 64 rows)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    b, vocab = rows.shape
    nxt, step = be.buf(np.zeros(b, np.int32)), be.buf(np.zeros(1, np.int32))
    pos, ctx, slots = be.buf(np.zeros(b, np.int32)), be.buf(np.zeros(b, np.uint32)), be.buf(np.zeros(b, np.int64))
    bt, scratch, xb = be.buf(np.zeros((b, 4), np.uint32)), be.buf(np.zeros(b, np.int64)), be.buf(rows)
    rc = be.sym("mrs_sample_greedy_advance", [VP, I, I, VP, VP, I, VP, VP, VP, VP, VP, I, I, VP, VP], I)(
        xb.ptr, vocab, b, nxt.ptr, None, 0, step.ptr, pos.ptr, ctx.ptr, slots.ptr, bt.ptr, 4, 32, scratch.ptr, be.stream or None)
    assert rc == 0
    return nxt.numpy().astype(np.int64)


@functools.lru_cache(maxsize=None)
def _rows(n, seed, rows=8):
    x = (np.random.default_rng(seed).standard_normal((rows, n)) * 3).astype(np.float32)
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------- greedy, exact
GREEDY_SHAPES = [(2051, 2048), (5000, 1000), (128256, 2048)]


def check_greedy(be, vocab, chunk):
    """every n in {0, 1, 4, 7}: all drafts match, and the first mismatch at each index -- all of them sequences of ONE launch (mixed n, 0 and 7 included); planted NaN
    rows after the deciding row change nothing"""
    base = _rows(vocab, vocab)
    win = base.argmax(axis=1)
    tgt, ids, seq_rows, want = [], [], [0], []
    for n in (0, 1, 4, 7):
        for miss in [None] + list(range(n)):
            d = [int(win[i]) for i in range(n)]
            if miss is not None:
                d[miss] = (d[miss] + 1) % vocab
            r = base[:n + 1].copy()
            if miss is not None and miss + 1 <= n:
                r[miss + 1:] = np.nan  # rows after the deciding row
            tgt.append(r)
            ids += d + [-5]
            seq_rows.append(seq_rows[-1] + n + 1)
            acc = n if miss is None else miss
            want.append((acc, d[:acc] + [int(win[acc])]))
    na, ot = run_verify(be, np.concatenate(tgt), ids, seq_rows, GREEDY, 1.0, None, chunk)
    for s, (acc, toks) in enumerate(want):
        assert na[s] == acc and ot[s, :acc + 1].tolist() == toks and np.all(ot[s, acc + 1:] == -1), (s, na[s], ot[s], acc, toks)
    # the same sequences without the NaN rows: identical
    clean = np.concatenate([base[:t.shape[0]] for t in tgt])
    na2, ot2 = run_verify(be, clean, ids, seq_rows, GREEDY, 1.0, None, chunk)
    assert np.array_equal(na, na2) and np.array_equal(ot, ot2)
    # a NaN IN the deciding row is reported
    bad = base[:2].copy()
    bad[1, vocab - 1] = np.nan
    na, ot = run_verify(be, bad, [int(win[0]), 0], [0, 2], GREEDY, 1.0, None, chunk)
    assert na[0] == -1 and np.all(ot[0] == -1)


def check_greedy_ties(be, vocab, chunk):
    """winners equal mrs_sample_greedy_advance's on ties, -0.0 / +0.0 pairs and -inf fill"""
    r = np.full((6, vocab), NINF, np.float32)
    r[0, [5, vocab - 1]] = 1.0                      # a tie across chunks: the lower index
    r[1, :] = -0.0
    r[1, 7] = 0.0                                   # -0.0 ranks with +0.0: index 0
    r[2, 3], r[2, 2] = -0.0, 0.0
    r[3, vocab - 2], r[3, vocab - 3] = 0.0, -0.0
    r[4, chunk - 1], r[4, min(chunk, vocab - 1)] = -3.5, -3.5  # a tie at the chunk edge, everything else -inf
    r[5] = _rows(vocab, 3)[0]
    r[5, [11, 4000 % vocab]] = r[5].max() + 1
    ref = greedy_advance_winners(be, r)
    assert ref[:4].tolist() == [5, 0, 2, vocab - 3] and ref[4] == chunk - 1
    na, ot = run_verify(be, r, [0] * 6, list(range(7)), GREEDY, 1.0, None, chunk)  # six sequences without drafts
    assert np.all(na == 0) and np.array_equal(ot[:, 0], ref), (ot[:, 0], ref)
    # as drafts of one sequence: all accepted, the sixth row is the bonus row
    na, ot = run_verify(be, r, ref.tolist()[:5] + [0], [0, 6], GREEDY, 1.0, None, chunk)
    assert na[0] == 5 and ot[0, :6].tolist() == ref.tolist()


# ---------------------------------------------------------------- temperature, exact
def _p_of(x, inv_t):
    z = x.astype(np.float64) * np.float64(np.float32(inv_t))
    z -= z.max()
    p = np.exp(z)
    return p / p.sum()


def check_temperature_exact(be, vocab, chunk):
    x = _rows(vocab, vocab + 1)
    inv_t = np.float32(1.0 / 0.8)
    p0 = _p_of(x[0], inv_t)
    d = int(np.argsort(p0)[-2])  # a token with a sizeable probability that is not 1
    # draft_logits NULL: accepted iff u0 < p_d; a rejection never returns the draft
    u0s = [0.0, p0[d] * 0.5, p0[d] * 0.999, p0[d] * 1.001, 0.5 + p0[d] / 2, U_TOP]
    u1s = [0.0, 0.3, 0.6, 0.9, U_TOP, p0[d]]
    tgt = np.concatenate([x[:2]] * len(u0s))
    us = np.zeros((2 * len(u0s), 2), np.float32)
    us[0::2, 0], us[0::2, 1], us[1::2, 1] = u0s, u1s, u1s
    na, ot = run_verify(be, tgt, [d, 0] * len(u0s), list(range(0, 2 * len(u0s) + 1, 2)), TEMP, inv_t, us, chunk)
    for s, u0 in enumerate(u0s):
        if np.float32(u0) < p0[d] * (1 - 1e-5):
            assert na[s] == 1 and ot[s, 0] == d, (s, na[s], ot[s])
        elif np.float32(u0) > p0[d] * (1 + 1e-5):
            assert na[s] == 0 and ot[s, 0] != d and 0 <= ot[s, 0] < vocab, (s, na[s], ot[s])
    # the residual of a deterministic proposer over ALL of u1: never the draft, even when the draft holds nearly all of p
    peaked = np.full((2, vocab), -30.0, np.float32)
    peaked[0, d], peaked[0, vocab - 1] = 10.0, -5.0
    grid = ((np.arange(64) + 0.5) / 64).astype(np.float32)
    us = np.zeros((128, 2), np.float32)
    us[0::2, 0], us[0::2, 1] = U_TOP, grid
    na, ot = run_verify(be, np.concatenate([peaked] * 64), [d, 0] * 64, list(range(0, 129, 2)), TEMP, 1.0, us, chunk)
    assert np.all(na == 0) and np.all(ot[:, 0] != d) and np.all(ot[:, 0] >= 0), ot[:, 0]
    # draft_logits bit-equal to the target: accepted for every u0 < 1
    us = np.zeros((8, 2), np.float32)
    us[0::2, 0] = [0.0, 0.5, 0.999, U_TOP]
    us[1::2, 1] = 0.4
    tgt = np.concatenate([x[:2]] * 4)
    na, ot = run_verify(be, tgt, [d, 0, 17, 0, vocab - 1, 0, int(p0.argmin()), 0], [0, 2, 4, 6, 8], TEMP, inv_t, us, chunk, draft=tgt)
    assert np.all(na == 1), na
    # all accepted: the bonus token is the categorical draw on that row at u1
    pk, _, _ = run_cat(be, x[1:2], inv_t, [0.4], chunk)
    assert np.all(ot[:, 1] == int(pk[0, 0]))
    # q_d = 0 and p_d > 0: accepted; p_d = 0: rejected at u0 = 0; p_d = q_d = 0 with p == q: the residual is empty, the token is the categorical draw from p at u1
    t = x[:2].copy()
    q = x[:2].copy()
    q[0, 5] = NINF
    us = np.array([[U_TOP, 0.1], [0.0, 0.25]], np.float32)
    na, ot = run_verify(be, t, [5, 0], [0, 2], TEMP, inv_t, us, chunk, draft=q)
    assert na[0] == 1 and ot[0, 0] == 5, (na, ot)
    t[0, 5] = NINF
    us = np.array([[0.0, 0.6], [0.0, 0.25]], np.float32)
    na, ot = run_verify(be, t, [5, 0], [0, 2], TEMP, inv_t, us, chunk, draft=None)
    assert na[0] == 0 and ot[0, 0] != 5, (na, ot)
    na, ot = run_verify(be, t, [5, 0], [0, 2], TEMP, inv_t, us, chunk, draft=t)  # p == q bit for bit, both 0 at the draft
    pk, _, _ = run_cat(be, t[0:1], inv_t, [0.6], chunk)
    assert na[0] == 0 and ot[0, 0] == int(pk[0, 0]) and ot[0, 0] != 5, (na, ot, pk)
    # no drafts: the plain draw
    na, ot = run_verify(be, t[0:1], [0], [0, 1], TEMP, inv_t, [[0.0, 0.6]], chunk)
    assert na[0] == 0 and ot[0, 0] == int(pk[0, 0])


def check_unusable(be, vocab, chunk):
    """an unusable deciding row reports -1; the good sequences beside it are what they are alone"""
    x = _rows(vocab, vocab + 2)
    d = int(x[0].argmax())
    good = x[:2]
    with_nan, with_inf = good.copy(), good.copy()
    with_nan[0, vocab - 1] = np.nan
    with_inf[0, 3] = np.inf
    nan_later = good.copy()
    nan_later[1] = np.nan  # after the deciding row when the draft is rejected
    seqs = [good, with_nan, good, with_inf, good, good, good, nan_later, good]
    inv_t = [1.0, 1.0, 1.0, 1.0, 0.0, np.inf, 1.0, 1.0, 1.0]
    u = [[U_TOP, 0.3], [0.1, 0.3], [0.0, 0.3], [0.1, 0.3], [0.1, 0.3], [0.1, 0.3], [1.0, 0.3], [U_TOP, 0.7], [U_TOP, 1.5]]
    bad = [1, 3, 4, 5, 6, 8]
    us = np.zeros((2 * len(seqs), 2), np.float32)
    us[0::2] = u
    us[1::2, 1] = 0.5
    ids = [d, 0] * len(seqs)
    na, ot = run_verify(be, np.concatenate(seqs), ids, list(range(0, 2 * len(seqs) + 1, 2)), TEMP, inv_t, us, chunk)
    for s in range(len(seqs)):
        if s in bad:
            assert na[s] == -1 and np.all(ot[s] == -1), (s, na[s], ot[s])
        else:
            a1, o1 = run_verify(be, seqs[s], [d, 0], [0, 2], TEMP, inv_t[s], us[2 * s:2 * s + 2], chunk)
            assert na[s] == a1[0] >= 0 and np.array_equal(ot[s], o1[0]), (s, na[s], ot[s], a1, o1)
    assert na[0] == 0 and na[2] == 1 and na[7] == 0
    # a sequence with an unknown mode, and one whose row count is outside 1..8
    na, ot = run_verify(be, np.concatenate([good, good]), [d, 0, d, 0], [0, 2, 4], [2, TEMP], 1.0, us[:4], chunk)
    assert na[0] == -1 and na[1] >= 0


def check_refusals(be):
    """the launcher returns without writing: more than 8 rows for the sequences, no sequence, a workspace that is too small"""
    x = np.zeros((9, 100), np.float32)
    for kw in (dict(), dict(nseq=0), dict(ws_cut=1)):
        rows = 9 if not kw else 2
        seq_rows = [0, rows]
        na, ot = run_verify(be, x[:rows], [0] * rows, seq_rows, GREEDY, 1.0, None, 64, **kw)
        assert na[0] == KEEP and np.all(ot == KEEP), (kw, na, ot)
    na, ot = run_verify(be, x[:8], [0] * 8, [0, 8], GREEDY, 1.0, None, 64)
    assert na[0] == 7 and ot[0].tolist() == [0] * 8


# ---------------------------------------------------------------- admissibility against float64 (tests/test_categorical.py part B: eps and the ambiguous-share cap)
ADM_SHAPES = [(2051, 2048, 0.5, 11), (5000, 1000, 1.0, 12), (128256, 2048, 0.7, 13)]
GRID = 256  # uniforms per sweep on the device; the host emulation (seconds per hundred workgroups) sweeps HOST_GRID of them under the same definitions
HOST_GRID = 16


def _exact_rule(xt, xq, d, inv_t):
    p, q = _p_of(xt, inv_t), _p_of(xq, inv_t)
    accept = min(1.0, p[d] / q[d])
    res = np.maximum(p - q, 0.0)
    return accept, np.cumsum(res) / res.sum()


def _pick_draft(xt, xq, inv_t):
    """a draft the proposer likes whose accept probability lies strictly inside (0, 1): both decisions occur on a grid of u0"""
    p, q = _p_of(xt, inv_t), _p_of(xq, inv_t)
    ratio = np.minimum(1.0, p / q)
    return next(int(t) for t in np.argsort(q)[::-1] if 0.05 < ratio[t] < 0.95)


def _ambiguous_share(cdf, us, eps):
    te = np.minimum(np.searchsorted(cdf, us, side="right"), cdf.size - 1)
    lo = np.where(te > 0, cdf[np.maximum(te - 1, 0)], 0.0)
    return te, (us - lo > eps) & (cdf[te] - us > eps)


def check_admissible(be, n, chunk, temp, seed, GRID=GRID):
    rng = np.random.default_rng(seed)
    xt, xq = (rng.standard_normal(n) * 3).astype(np.float32), (rng.standard_normal(n) * 3).astype(np.float32)
    inv_t = np.float32(1.0 / temp)
    nb = (n + chunk - 1) // chunk
    eps = (nb + 32) * 2.0 ** -23
    grid = ((np.arange(GRID) + 0.5) / GRID).astype(np.float32)
    d = _pick_draft(xt, xq, inv_t)
    accept, cdf = _exact_rule(xt, xq, d, inv_t)
    tgt = np.broadcast_to(np.stack([xt, xt]), (GRID, 2, n)).reshape(2 * GRID, n)
    drf = np.broadcast_to(np.stack([xq, xq]), (GRID, 2, n)).reshape(2 * GRID, n)
    seq_rows = list(range(0, 2 * GRID + 1, 2))
    # (1) the accept decision over a grid of u0
    us = np.zeros((2 * GRID, 2), np.float32)
    us[0::2, 0], us[:, 1] = grid, 0.5
    na, ot = run_verify(be, tgt, [d, 0] * GRID, seq_rows, TEMP, inv_t, us, chunk, draft=drf)
    clear = np.abs(grid.astype(np.float64) - accept) > eps
    assert clear.mean() >= 1 - MAX_AMBIGUOUS
    assert np.all(na >= 0) and np.array_equal(na[clear] == 1, grid[clear].astype(np.float64) < accept), "the accept decision differs from exact arithmetic"
    # (2) the rejection token over a grid of u1 (u0 at the top of [0, 1): rejected, accept < 0.95)
    us[0::2, 0], us[0::2, 1] = U_TOP, grid
    na, ot = run_verify(be, tgt, [d, 0] * GRID, seq_rows, TEMP, inv_t, us, chunk, draft=drf)
    assert np.all(na == 0)
    t = ot[:, 0]
    u1 = grid.astype(np.float64)
    assert np.all((t >= 0) & (t < n))
    lo = np.where(t > 0, cdf[np.maximum(t - 1, 0)], 0.0)
    ok = (lo - eps <= u1) & (u1 < cdf[t] + eps)
    assert ok.all(), f"{(~ok).sum()} rejection tokens outside the exact interval +- eps"
    te, clear = _ambiguous_share(cdf, u1, eps)
    print(f"n={n} chunk={chunk}: accept {accept:.4f}, ambiguous {(~clear).sum()}/{GRID}, tokens off the exact one {(t != te).sum()}")
    assert (~clear).mean() <= MAX_AMBIGUOUS, "the float64 rule alone leaves too many rows ambiguous: pick another seed"
    assert np.array_equal(t[clear], te[clear]), f"{(t[clear] != te[clear]).sum()} unambiguous rows drew another token than exact arithmetic"
    assert np.all(np.diff(t) >= 0)
    # the host statement of the rule is admissible in the same sense
    # (one chunk of n sequential additions: the same eps formula with n in the place of the chunk count, as tests/test_categorical.py holds categorical_host to)
    if n <= 5000:
        from mistralrs_amd import speculative
        clear_h = _ambiguous_share(cdf, u1, (n + 32) * 2.0 ** -23)[1]
        for j in range(0, GRID, max(1, GRID // 16)):
            acc_h, toks = speculative.verify_host(np.stack([xt, xt]), [d], temp, [[U_TOP, grid[j]], [0, 0.5]], draft_rows=np.stack([xq, xq]))
            assert acc_h == 0 and (toks[0] == te[j] or not clear_h[j])


@pytest.mark.parametrize("n,chunk,temp,seed", ADM_SHAPES[:2], ids=[f"n{s[0]}c{s[1]}" for s in ADM_SHAPES[:2]])
def test_admissible_seeds_leave_few_ambiguous_rows(n, chunk, temp, seed):
    """CPU: for the seeds above the float64 rule alone keeps the ambiguous share under the cap (the device tests assert it again on their own grid)"""
    rng = np.random.default_rng(seed)
    xt, xq = (rng.standard_normal(n) * 3).astype(np.float32), (rng.standard_normal(n) * 3).astype(np.float32)
    inv_t = np.float32(1.0 / temp)
    eps = ((n + chunk - 1) // chunk + 32) * 2.0 ** -23
    d = _pick_draft(xt, xq, inv_t)
    accept, cdf = _exact_rule(xt, xq, d, inv_t)
    grid = ((np.arange(GRID) + 0.5) / GRID).astype(np.float64)
    assert (~_ambiguous_share(cdf, grid, eps)[1]).mean() <= MAX_AMBIGUOUS and (np.abs(grid - accept) <= eps).mean() <= MAX_AMBIGUOUS
    # ... and on these seeds the host statement of the rule takes the exact decision and draws the exact token wherever its own eps (n sequential additions) leaves no doubt
    from mistralrs_amd import speculative
    te, clear_h = _ambiguous_share(cdf, grid, (n + 32) * 2.0 ** -23)
    rows, drows = np.stack([xt, xt]), np.stack([xq, xq])
    for j in range(0, GRID, 32):
        u = np.float32(grid[j])
        acc_h, toks = speculative.verify_host(rows, [d], temp, [[u, 0.5], [0, 0.5]], draft_rows=drows)
        assert abs(u - accept) <= eps or acc_h == int(u < accept)
        acc_h, toks = speculative.verify_host(rows, [d], temp, [[U_TOP, u], [0, 0.5]], draft_rows=drows)
        assert acc_h == 0 and (toks[0] == te[j] or not clear_h[j])


# ---------------------------------------------------------------- the law
def check_law(be, G=64):
    """vocab 6, one draft per sequence: for every draft d the uniforms (u0, u1) sweep the midpoints of a G x G grid (64 x 64 on the device); the emitted-token frequencies
    weighted by q(d) equal p within 1/G + 1/G per token (one grid cell of u0 at the accept boundary, one of u1 at a residual boundary)"""
    p = np.array([0.35, 0.05, 0.25, 0.0, 0.2, 0.15])
    q = np.array([0.1, 0.3, 0.25, 0.2, 0.0, 0.15])
    with np.errstate(divide="ignore"):
        xt, xq = np.log(p).astype(np.float32), np.log(q).astype(np.float32)
    g = ((np.arange(G) + 0.5) / G).astype(np.float32)
    u0, u1 = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    cells = u0.size
    nseq = 6 * cells
    tgt = np.broadcast_to(np.stack([xt, xt]), (nseq, 2, 6)).reshape(2 * nseq, 6)
    drf = np.broadcast_to(np.stack([xq, xq]), (nseq, 2, 6)).reshape(2 * nseq, 6)
    us = np.zeros((2 * nseq, 2), np.float32)
    us[0::2, 0], us[0::2, 1] = np.tile(u0, 6), np.tile(u1, 6)
    us[1::2, 1] = 0.5
    ids = np.zeros(2 * nseq, np.int32)
    ids[0::2] = np.repeat(np.arange(6), cells)
    na, ot = run_verify(be, tgt, ids, list(range(0, 2 * nseq + 1, 2)), TEMP, 1.0, us, 4, draft=drf)  # two chunks: 4 + 2 tokens
    assert np.all(na >= 0)
    first = ot[:, 0].reshape(6, cells)
    assert np.all((first >= 0) & (first < 6))
    # cell by cell: the emitted token is the float64 rule's.  No midpoint of a 4 .. 64 grid lies within 1e-5 of the accept probabilities (1, 1/6, 1, 0, 1, 1) or of the
    # residual's one inner boundary (0.25 / 0.45), so EVERY cell must agree: this holds at any G, the law's 2 / G bound below is then a property of the grid alone
    res = np.maximum(p - q, 0.0)
    rcdf = np.cumsum(res) / res.sum()
    for d in range(6):
        accept = min(1.0, p[d] / q[d]) if q[d] > 0 else float(p[d] > 0)
        assert np.all(np.abs(u0.astype(np.float64) - accept) > 1e-5) and np.all(np.abs(u1.astype(np.float64)[:, None] - rcdf[None, :-1]) > 1e-5)
        want = np.where(u0 < accept, d, np.searchsorted(rcdf, u1.astype(np.float64), side="right"))
        assert np.array_equal(first[d], want), (d, np.nonzero(first[d] != want)[0][:5])
    freq = np.stack([np.bincount(first[d], minlength=6) / cells for d in range(6)])  # [draft][emitted token]
    law = q @ freq
    assert np.abs(law - p).max() <= 1 / G + 1 / G, (law, p)
    assert not np.any(first == 3) and np.all(first[4] == 4)  # p(3) = 0: never emitted; q(4) = 0 < p(4): a forced draft of 4 is always accepted (and weighs nothing)


# ---------------------------------------------------------------- the state advance
def run_advance(be, n_acc, toks, seq, step, pos, stride, max_blocks, b=2):
    ids, tout, stepb = be.buf(np.full(b, 90, np.int32)), be.buf(np.full(b * stride, -7, np.int32)), be.buf(np.array([step], np.int32))
    posb, ctx, slots = be.buf(np.full(b, pos, np.int32)), be.buf(np.full(b, pos + 1, np.uint32)), be.buf(np.full(b, 123, np.int64))
    bt = be.buf((100 + np.arange(b * max_blocks)).astype(np.uint32))
    nb_, tb = be.buf(np.array([n_acc], np.int32)), be.buf(np.asarray(toks, dtype=np.int32))
    rc = be.sym("mrs_spec_advance", [VP, VP, I, VP, VP, I, VP, VP, VP, VP, VP, I, I, VP], I)(
        nb_.ptr, tb.ptr, seq, ids.ptr, tout.ptr, stride, stepb.ptr, posb.ptr, ctx.ptr, slots.ptr, bt.ptr, max_blocks, 32, be.stream or None)
    assert rc == 0
    return dict(ids=ids.numpy(), tout=tout.numpy().reshape(b, stride), step=int(stepb.numpy()[0]), pos=posb.numpy(), ctx=ctx.numpy(), slots=slots.numpy())


def check_advance(be):
    toks = [11, 12, 13, 14, 15, 16, 17, 18]
    for n_acc, pos in ((0, 5), (3, 29), (7, 30)):  # 29 + 4 and 30 + 8 cross the 32-token block edge
        r = run_advance(be, n_acc, toks, 1, 4, pos, 40, 3)
        new = pos + n_acc + 1
        assert r["tout"][1, 4:5 + n_acc].tolist() == toks[:n_acc + 1] and np.all(r["tout"][1, 5 + n_acc:] == -7) and np.all(r["tout"][0] == -7)
        assert r["step"] == 5 + n_acc and r["ids"].tolist() == [90, toks[n_acc]]
        assert r["pos"].tolist() == [pos, new] and r["ctx"].tolist() == [pos + 1, new + 1]
        assert r["slots"].tolist() == [123, (100 + 3 + new // 32) * 32 + new % 32]
    r = run_advance(be, 7, toks, 0, 36, 10, 40, 3, b=1)  # tokens past tokens_out_stride are dropped; the counter still counts them
    assert r["tout"][0, 36:].tolist() == toks[:4] and r["step"] == 44
    r = run_advance(be, 3, toks, 0, 0, 93, 40, 3, b=1)  # position 97 lies past the 3-block table
    assert r["slots"][0] == -1 and r["pos"][0] == 97 and r["ctx"][0] == 98
    r = run_advance(be, -1, toks, 0, 2, 10, 40, 3, b=1)  # an unusable round changes nothing
    assert r["step"] == 2 and r["pos"][0] == 10 and r["ids"][0] == 90 and np.all(r["tout"] == -7) and r["slots"][0] == 123


# ---------------------------------------------------------------- the host statement of the rule (no device)
def test_verify_host_states_the_rule():
    from mistralrs_amd import sampler, speculative
    x = _rows(2051, 1)
    win = x.argmax(axis=1)
    assert speculative.verify_host(x[:5], win[:4]) == (4, win[:5].tolist())
    assert speculative.verify_host(x[:5], [win[0], win[1], 0, win[3]]) == (2, [int(win[0]), int(win[1]), int(win[2])])
    z = np.full((1, 9), -0.0, np.float32)
    z[0, 4] = 0.0
    assert speculative.verify_host(z, []) == (0, [0])
    with pytest.raises(ValueError):
        speculative.verify_host(np.full((1, 9), np.nan, np.float32), [])
    p0 = _p_of(x[0], 1.0)
    d = int(win[0])
    assert speculative.verify_host(x[:2], [d], 1.0, [[p0[d] * 0.99, 0.3], [0, 0.4]]) == (1, [d, sampler.categorical_host(x[1], 1.0, 0.4)[0]])
    acc, toks = speculative.verify_host(x[:2], [d], 1.0, [[min(p0[d] * 1.01, U_TOP), 0.3], [0, 0.4]])
    assert acc == 0 and toks[0] != d
    assert speculative.verify_host(x[:2], [7], 1.0, [[U_TOP, 0.3], [0, 0.4]], draft_rows=x[:2])[0] == 1
    with pytest.raises(ValueError):
        speculative.verify_host(x[:2], [d], 1.0, [[1.0, 0.3], [0, 0.4]])
    ng = speculative.NGramProposer(3, 4)
    assert ng.propose([1, 2, 3, 4, 5, 9, 2, 3, 4], 7)[0] == [5, 9, 2, 3]
    assert ng.propose([1, 2, 3, 4, 5, 9, 2, 3, 4], 2)[0] == [5, 9]
    assert ng.propose([1, 2, 3], 4)[0] == []
    assert ng.propose([7, 8, 7, 8, 7], 4)[0] == [8, 7]  # the most recent earlier occurrence of (8, 7)


# ---------------------------------------------------------------- the code object
def test_spec_kernels_no_scratch_no_spills():
    lib = os.path.join(ROOT, "mistral.rs_amd", "lib", "libmistralrscuda.so")
    if not os.path.exists(lib):
        pytest.skip("libmistralrscuda.so not built (python mistral.rs_amd/build.py)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    ks = [k for k in m.resources(lib) if "spec_" in k["demangled"] or "spec_" in k["name"]]
    names = " ".join(k["demangled"] for k in ks)
    for want in ("spec_stage1_kernel", "spec_decide_kernel", "spec_residual_kernel", "spec_resolve_kernel"):
        assert want in names, (want, names)
    bad = [(k["demangled"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count")) for k in ks
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0)]
    assert not bad, bad
    # the state advance and the verify step's gather live in the runner's library
    ext = os.path.join(ROOT, "mistral.rs_amd", "lib", "libmrs_hip_ext.so")
    assert os.path.exists(ext), "libmrs_hip_ext.so not built"
    ks = [k for k in m.resources(ext) if "spec_advance_kernel" in k["demangled"] + k["name"] or "spec_prep_kernel" in k["demangled"] + k["name"]]
    assert len(ks) == 2, [k["demangled"] for k in ks]
    bad = [(k["demangled"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count")) for k in ks
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0)]
    assert not bad, bad


# ---------------------------------------------------------------- the two backends
@pytest.fixture(scope="module")
def host():
    from tests.abi_backends import HostBackend
    return HostBackend()


@pytest.fixture(scope="module")
def gpu(dev):
    from tests.abi_backends import GpuBackend
    return GpuBackend(dev)


HOST_SHAPES = GREEDY_SHAPES[:2]
_ids = lambda shapes: [f"n{s[0]}c{s[1]}" for s in shapes]


@pytest.mark.parametrize("vocab,chunk", HOST_SHAPES, ids=_ids(HOST_SHAPES))
def test_greedy_host_emulation(host, vocab, chunk):
    check_greedy(host, vocab, chunk)
    check_greedy_ties(host, vocab, chunk)


@pytest.mark.parametrize("vocab,chunk", HOST_SHAPES, ids=_ids(HOST_SHAPES))
def test_temperature_exact_host_emulation(host, vocab, chunk):
    check_temperature_exact(host, vocab, chunk)
    check_unusable(host, vocab, chunk)


@pytest.mark.parametrize("n,chunk,temp,seed", ADM_SHAPES[:2], ids=_ids(ADM_SHAPES[:2]))
def test_admissible_host_emulation(host, n, chunk, temp, seed):
    check_admissible(host, n, chunk, temp, seed, GRID=2 * HOST_GRID if n < 4096 else HOST_GRID)  # about the same number of chunk workgroups either way


def test_law_host_emulation(host):
    # 96 sequences on host fibers within seconds.  What checks the kernels here is check_law's cell-by-cell comparison with the float64 rule (a wrong accept decision or
    # residual inversion fails it); at G = 4 the 2 / G assertion on the frequencies adds nothing to that.  The 64 x 64 grid and its 1/32 bound run on the device.
    check_law(host, G=4)


def test_advance_host_emulation(host):
    check_advance(host)


def test_refusals_host_emulation(host):
    check_refusals(host)


@pytest.mark.gpu
@pytest.mark.parametrize("vocab,chunk", GREEDY_SHAPES, ids=_ids(GREEDY_SHAPES))
def test_greedy_gpu(gpu, vocab, chunk):
    check_greedy(gpu, vocab, chunk)
    check_greedy_ties(gpu, vocab, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("vocab,chunk", GREEDY_SHAPES, ids=_ids(GREEDY_SHAPES))
def test_temperature_exact_gpu(gpu, vocab, chunk):
    check_temperature_exact(gpu, vocab, chunk)
    check_unusable(gpu, vocab, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunk,temp,seed", ADM_SHAPES, ids=_ids(ADM_SHAPES))
def test_admissible_gpu(gpu, n, chunk, temp, seed):
    check_admissible(gpu, n, chunk, temp, seed)


@pytest.mark.gpu
def test_law_gpu(gpu):
    check_law(gpu)


@pytest.mark.gpu
def test_advance_gpu(gpu):
    check_advance(gpu)


@pytest.mark.gpu
def test_refusals_gpu(gpu):
    check_refusals(gpu)
