"""The bf16-shadow prompt path at kernel level: what the runner's calls reach and the model-level tolerances cannot see.
  A. prefill_attn_kernel (csrc/ext_attn_prefill.hip) through mrs_prefill_attention_window_f32_bf16 with a sliding window, chunk starts > 0 (the per-tile skip of
     old key blocks) and the runner's row strides (q = a column range of the fused qkv GEMM output), against a plain f64 restatement of the reference's rule
     (paged_attention/layers/paged_attention.rs:551-553: a query at p attends keys (p - W, p]).  Every query carries a planted key at p - W, p - W + 1 or p + 1
     whose logit is raised by 8: one wrongly included or excluded key moves the output by far more than the tolerance -- asserted on the reference itself.
  B. the small row producers and folds of the same path: mrs_rows_rms_norm_bf16 / mrs_rows_glu_bf16 (csrc/ext_gemm_lt.hip, GPU only: that file needs hipBLASLt) to
     half a bf16 ulp of the f64 value, mrs_resid_scale_add_f32 / mrs_vec_add_f32 bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.abi_backends import GpuBackend, HostBackend

VP, CI = C.c_void_p, C.c_int
HD, BS = 128, 32
PW = [VP, VP, VP, VP, VP] + [CI] * 10 + [C.c_float, CI, VP]  # mrs_prefill_attention_window_f32_bf16
SENTINEL = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]  # finite; compared as bits
BOOST = 8.0  # logit of the planted key is raised by this much
SCALE = 1.0 / np.sqrt(HD)

#                (T, start, W, heads, kvh)
WINDOW_CASES = [(70, 0, 40, 8, 2),       # the window bites inside the first chunk; kb0 stays 0: the mask alone
                (96, 160, 100, 8, 1),    # kb0 > 0 and different per tile, G = 8; a tile's first processed block is fully masked for its later queries
                (33, 300, 64, 4, 4),     # G = 1, partial second tile, W a multiple of the block size
                (40, 1000, 32, 16, 2),   # W == block size, deep chunk start (kb0 about 30)
                (37, 500, 33, 2, 2),     # W == block size + 1
                (37, 511, 33, 2, 2),     # first_q_pos - W + 1 is the last slot of a block: block kb0 holds one live key, that of the tile's first query
                (65, 31, 1, 4, 2),       # W = 1: each query attends itself only
                (50, 20, 4096, 4, 1),    # W larger than the sequence: same as no window
                (64, 45, 0, 16, 2)]      # W = 0 through the window entry point, strided: the causal p + 1 plant
GPU_CASES = WINDOW_CASES + [(200, 4000, 1024, 32, 8)]  # Llama / Mistral grouping, a window spanning 32 blocks


def _reference(qb, k, v, start, variants):
    """f64 attention of queries at positions start .. start+T-1 over keys 0 .. start+T-1.  variants: (W, future) pairs; W = 0: causal only; future: every query also
    sees key p + 1 (a deliberately wrong rule, for the sensitivity condition).  q already bf16-rounded; p = e / (sum + 1e-6) rounded to bf16, then p @ v.
    Returns {variant: out [T][heads][hd]} and, for the FIRST variant, sum_t p_t |v_t| with the unrounded p."""
    T, heads, _ = qb.shape
    S, kvh, _ = k.shape
    G = heads // kvh
    pos = start + np.arange(T)[:, None]
    kpos = np.arange(S)[None, :]
    masks = [(kpos <= pos + (1 if fut else 0)) & ((kpos > pos - W) if W > 0 else True) for W, fut in variants]
    outs = [np.zeros((T, heads, HD)) for _ in variants]
    pabs = np.zeros((T, heads, HD))
    k64, v64 = k.astype(np.float64), v.astype(np.float64)
    for h in range(heads):
        s = SCALE * (qb[:, h].astype(np.float64) @ k64[:, h // G].T)  # [T][S]
        for i, mask in enumerate(masks):
            sm = np.where(mask, s, -np.inf)
            e = np.exp(sm - sm.max(axis=1, keepdims=True))
            p = e / (e.sum(axis=1, keepdims=True) + 1e-6)
            outs[i][:, h] = O.round_bf16(p.astype(np.float32)).astype(np.float64) @ v64[:, h // G]
            if i == 0:
                pabs[:, h] = p @ np.abs(v64[:, h // G])
    return dict(zip(variants, outs)), pabs


@functools.lru_cache(maxsize=None)
def _case(T, start, W, heads, kvh):
    """Inputs, reference and tolerance of one case: built once, shared by the host-emulation and the GPU run, never written to."""
    rng = np.random.default_rng([T, start, W, heads, kvh])
    S, G = start + T, heads // kvh
    k = O.round_bf16(rng.standard_normal((S, kvh, HD)).astype(np.float32))
    v = O.round_bf16(rng.standard_normal((S, kvh, HD)).astype(np.float32))
    q = (2.0 * rng.standard_normal((T, heads, HD))).astype(np.float32)
    for t in range(T):
        p = start + t
        j = [p - W, p - W + 1, p + 1][t % 3] if W else p + 1  # newest excluded key / oldest included key / first future key
        if 0 <= j < S:
            kj = k[j].astype(np.float64)  # [kvh][hd]
            q[t] += np.repeat(BOOST * np.sqrt(HD) * kj / (kj * kj).sum(axis=1, keepdims=True), G, axis=0).astype(np.float32)
    # paged cache through a permuted block table: one spare table entry after the sequence's last block, three blocks no table entry names
    nbt = (S + BS - 1) // BS + 1
    nblocks = nbt + 3
    bt = rng.permutation(nblocks)[:nbt].astype(np.uint32)
    kc = O.round_bf16(rng.standard_normal((nblocks, kvh, HD // 8, BS, 8)).astype(np.float32))  # stale K: finite
    vc = np.full((nblocks, kvh, HD, BS), np.nan, np.float32)                                   # stale V: NaN
    blk, slot = bt[np.arange(S) // BS], np.arange(S) % BS
    kc[blk, :, :, slot, :] = k.reshape(S, kvh, HD // 8, 8)
    vc[blk, :, :, slot] = v
    assert np.isnan(vc[bt[-1]]).all() and np.isnan(vc).sum() == (nblocks * BS - S) * kvh * HD
    nq = heads * HD
    q_stride, o_stride = nq + 2 * kvh * HD, nq + 64
    qrows = rng.standard_normal((T, q_stride)).astype(np.float32)  # q = the first nq columns of the fused [T][nq + 2 nkv] row
    qrows[:, :nq] = q.reshape(T, nq)
    variants = [(W, False), (0, False), (W, True)]
    if W > 0:
        variants += [(W + 1, False)] + ([(W - 1, False)] if W > 1 else [])
    refs, pabs = _reference(O.round_bf16(q), k, v, start, tuple(variants))
    # test_paged_attn.py::test_prefill_attention: the kernel rounds the un-normalised p to bf16, the reference the normalised p, each within 2^-8 relative
    tol = 2.0 ** -7 * pabs + 1e-4 * np.abs(v).max()
    d = dict(T=T, start=start, W=W, heads=heads, kvh=kvh, k=k, v=v, bt=bt, kc=O.to_bf16_bits(kc), vc=O.to_bf16_bits(vc), qrows=qrows, q_stride=q_stride, o_stride=o_stride,
             want=refs[(W, False)], tol=tol, refs=refs)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _rows_differing(c, variant):
    """(query, head) rows on which the reference under `variant` leaves the case's own reference by more than 10 * tol somewhere"""
    return (np.abs(c["refs"][variant] - c["want"]) > 10 * c["tol"]).any(axis=2)


@pytest.mark.parametrize("T,start,W,heads,kvh", GPU_CASES)
def test_window_cases_are_sensitive(T, start, W, heads, kvh):
    """The reference alone: a window off by one in either direction, no window at all, or one future key each move the expected output by more than
    10 * tol on a good share of the rows -- so a kernel that passes check_window_prefill has the window and the causal edge exactly right."""
    c = _case(T, start, W, heads, kvh)
    fut = _rows_differing(c, (W, True))[:T - 1]  # the last query's p + 1 does not exist
    shares = {"future": fut.mean()}
    assert shares["future"] >= 0.25, shares
    if 0 < W <= start + T - 1:  # the window truncates at least one query
        for name, var, bar in [("W-1", (W - 1, False), 0.15), ("W+1", (W + 1, False), 0.15), ("none", (0, False), 0.30)]:
            if name != "W-1" or W > 1:
                shares[name] = _rows_differing(c, var).mean()
                assert shares[name] >= bar, (name, shares)
    elif W > 0:  # nothing truncated: the window changes nothing
        assert np.array_equal(c["refs"][(0, False)], c["want"])
    print(f"sensitivity {(T, start, W, heads, kvh)}: " + ", ".join(f"{n} {s:.2f}" for n, s in shares.items()))


def _run_window(be, c, W):
    T, heads, kvh = c["T"], c["heads"], c["kvh"]
    q, kc, vc, bt = be.buf(c["qrows"]), be.buf(c["kc"].view(np.int16)), be.buf(c["vc"].view(np.int16)), be.buf(c["bt"])
    out = be.buf(np.full((T + 1, c["o_stride"]), SENTINEL, np.float32))
    rc = be.sym("mrs_prefill_attention_window_f32_bf16", PW, CI)(q.ptr, kc.ptr, vc.ptr, bt.ptr, out.ptr, T, c["start"], heads, kvh, HD, BS, c["q_stride"], c["o_stride"],
                                                                 kvh * HD * BS, HD * BS, SCALE, W, be.stream)
    assert rc == 0, rc
    res = out.numpy()
    nq = heads * HD
    outside = np.ones(res.shape, bool)
    outside[:T, :nq] = False
    assert (res.view(np.uint32)[outside] == SENTINEL.view(np.uint32)).all(), "a store outside [0, T) x [0, heads * 128)"
    return res[:T, :nq].reshape(T, heads, HD)


def check_window_prefill(O, be, T, start, W, heads, kvh):
    """mrs_prefill_attention_window_f32_bf16 at positions start .. start+T-1 with window W, q at the fused-qkv row stride and out at its own, vs the f64 reference."""
    c = _case(T, start, W, heads, kvh)
    got = _run_window(be, c, W)
    assert np.isfinite(got).all(), f"{(~np.isfinite(got)).sum()} non-finite outputs: a stale V slot was read"
    err, tol = np.abs(got - c["want"]), c["tol"]
    print(f"window prefill {(T, start, W, heads, kvh)} on {be.name}: worst err / tol {float((err / tol).max()):.3f}")
    bad = np.argwhere(err > tol)
    assert len(bad) == 0, f"{len(bad)} outside tolerance, first (t, head, d) {bad[:6].tolist()} err {err[err > tol][:6]} tol {tol[err > tol][:6]}"
    if W == 1:  # each query attends itself only
        vp = np.repeat(c["v"][start:], heads // kvh, axis=1)
        assert (np.abs(got - vp) <= tol).all()
    if W > start + T:  # nothing truncated: the W = 0 call on the same buffers
        assert (np.abs(got - _run_window(be, c, 0)) <= tol).all()


@pytest.mark.parametrize("T,start,W,heads,kvh", WINDOW_CASES)
def test_window_prefill_host_emulation(oracle, T, start, W, heads, kvh):
    check_window_prefill(oracle, HostBackend(), T, start, W, heads, kvh)


@pytest.mark.gpu
@pytest.mark.parametrize("T,start,W,heads,kvh", GPU_CASES)
def test_window_prefill_gpu(oracle, dev, T, start, W, heads, kvh):
    check_window_prefill(oracle, GpuBackend(dev), T, start, W, heads, kvh)


def test_window_prefill_rejects_unsupported_shapes_host_emulation():
    """Every one of these returns before the launch: -1 for a shape the kernel does not serve (the caller falls back), 0 and no store for an empty chunk."""
    be = HostBackend()
    f = be.sym("mrs_prefill_attention_window_f32_bf16", PW, CI)
    kvh = 4
    q, kc, vc = be.buf(np.zeros((4, 8 * HD), np.float32)), be.buf(np.zeros((2, kvh, HD // 8, BS, 8), np.int16)), be.buf(np.zeros((2, kvh, HD, BS), np.int16))
    bt, out = be.buf(np.zeros(2, np.uint32)), be.buf(np.full((4, 8 * HD), SENTINEL, np.float32))

    def call(T=4, heads=8, kvh=kvh, hd=HD, bs=BS):
        return f(q.ptr, kc.ptr, vc.ptr, bt.ptr, out.ptr, T, 0, heads, kvh, hd, bs, 8 * HD, 8 * HD, kvh * hd * bs, hd * bs, SCALE, 2, None)
    assert call(hd=64) == -1
    assert call(bs=16) == -1
    assert call(heads=6, kvh=4) == -1
    assert call(heads=6, kvh=2) == -1  # G = 3
    assert call(T=0) == 0
    assert (out.numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()


# ------------------------------------------------------------------------------------------------ B. row producers (GPU only) and folds (both backends)
Y_SENTINEL = np.int16(-0x4111)  # 0xBEEF


def _half_ulp_bf16(want, extra_rel=0.0):
    """round-to-nearest-even to bf16 (8 significant bits) errs by at most half an ulp <= 2^-8 |want|; 2^-10 of that for the f32 arithmetic in front of the pack
    (about 1e-6 relative).  A truncating pack errs by up to 2^-7 |want| and fails."""
    return 2.0 ** -8 * np.abs(want) * (1 + 2.0 ** -10) + extra_rel * np.abs(want) + 1e-30


def _bf16_rows(buf, M):
    a = buf.numpy().view(np.uint16)
    assert (a[M:] == Y_SENTINEL.view(np.uint16)).all(), "a store past the last row"
    return O.from_bf16_bits(a[:M]).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(1, 8), (3, 520), (2, 4096), (257, 2056)])  # 520 and 2056: multiples of 8 that the 256-thread stride does not divide
def test_rows_rms_norm_bf16(dev, M, K):
    be = GpuBackend(dev)
    f = be.sym("mrs_rows_rms_norm_bf16", [VP, VP, CI, CI, C.c_float, VP, VP], CI)
    rng = np.random.default_rng(M * 10000 + K)
    eps = 1e-5
    w = (rng.random(K) + 0.5).astype(np.float32)
    for shift in range(3):  # every row magnitude at every row index, also when M < 3
        mag = np.array([1e-3, 1.0, 1e3])[(np.arange(M) + shift) % 3]
        x = (rng.standard_normal((M, K)) * mag[:, None]).astype(np.float32)
        y = be.buf(np.full((M + 1, K), Y_SENTINEL, np.int16))
        assert f(be.buf(x).ptr, be.buf(w).ptr, M, K, eps, y.ptr, be.stream) == 0
        x64 = x.astype(np.float64)
        want = x64 / np.sqrt((x64 * x64).mean(axis=1, keepdims=True) + np.float64(np.float32(eps))) * w.astype(np.float64)
        err, tol = np.abs(_bf16_rows(y, M) - want), _half_ulp_bf16(want)
        assert (err <= tol).all(), (shift, np.argwhere(err > tol)[:4].tolist(), float((err / tol).max()))
    assert f(None, None, 1, 12, eps, None, be.stream) == -1  # K % 8: returns before the launch


GLU_SHAPES = [(1, 8), (5, 264), (257, 1016)]
GLU_SPECIALS = np.array([0.0, -0.0, 30.0, -30.0, 100.0, -100.0, 1e-20], np.float32)
# the f32 arithmetic of g / (1 + expf(-g)) * u: twice the worst relative deviation of the NumPy float32 restatement from the f64 value at _glu_inputs
# (measured 2.279e-07; test_glu_f32_allowance_is_measured_on_the_restatement keeps the figure honest)
GLU_F32_REL = 4.6e-7


def _glu_inputs(M, N):
    """g and u as the two column halves of one [M][2N] buffer (gate_up_adjacent: ld = 2N); the special gates at the head of the first row and the tail of the last"""
    rng = np.random.default_rng(M * 10000 + N)
    gu = rng.standard_normal((M, 2 * N)).astype(np.float32)
    gu[:, :N] *= 4.0
    gu[0, :7] = GLU_SPECIALS
    if M > 1:
        gu[M - 1, N - 7:N] = GLU_SPECIALS[::-1]
    g64, u64 = gu[:, :N].astype(np.float64), gu[:, N:].astype(np.float64)
    return gu, g64 / (1.0 + np.exp(-g64)) * u64


def _glu_f32(gu, N):
    g, u = gu[:, :N], gu[:, N:]
    with np.errstate(over="ignore"):  # expf(100) = inf: g / inf = -0
        return g / (np.float32(1.0) + np.exp(-g)) * u


def test_glu_f32_allowance_is_measured_on_the_restatement():
    """GLU_F32_REL comes from the float32 restatement at the test's own inputs, never from the kernel: the constant is twice its worst relative deviation from f64
    (asserted loosely, between one and four times: NumPy's float32 exp may differ by an ulp between builds).
    Below the 1e-30 absolute floor of the bound (g = -100: expf overflows, the f32 value is -0 where f64 gives 4e-42 u) a relative figure means nothing."""
    worst = 0.0
    for M, N in GLU_SHAPES:
        gu, want = _glu_inputs(M, N)
        got = _glu_f32(gu, N).astype(np.float64)
        assert np.isfinite(got).all()
        big = np.abs(want) >= 1e-30
        assert (np.abs(got - want)[~big] <= 1e-30).all()
        worst = max(worst, float((np.abs(got - want)[big] / np.abs(want)[big]).max()))
    print(f"float32 restatement of SiLU(g) * u vs f64: worst relative deviation {worst:.3e}")
    assert worst <= GLU_F32_REL <= 4 * worst


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", GLU_SHAPES)
def test_rows_glu_bf16(dev, M, N):
    be = GpuBackend(dev)
    f = be.sym("mrs_rows_glu_bf16", [VP, VP, CI, CI, CI, VP, VP], CI)
    gu_np, want = _glu_inputs(M, N)
    gu = be.buf(gu_np)
    y = be.buf(np.full((M + 1, N), Y_SENTINEL, np.int16))
    assert f(gu.ptr, gu.ptr + 4 * N, 2 * N, M, N, y.ptr, be.stream) == 0
    got = _bf16_rows(y, M)
    assert np.isfinite(got).all()
    overflow = gu_np[:, :N] == -100.0  # expf overflows to inf: -100 / inf * u is a zero of either sign, not NaN
    assert overflow.sum() == min(M, 2) and (got[overflow] == 0.0).all()
    err, tol = np.abs(got - want), _half_ulp_bf16(want, GLU_F32_REL)
    assert (err <= tol).all(), (np.argwhere(err > tol)[:4].tolist(), float((err / tol).max()))
    assert f(None, None, 24, 1, 12, None, be.stream) == -1  # N % 8: returns before the launch


FOLD_N = [1, 3, 4, 5, 1023, 1027, 2048 * 1024 + 7]  # the last: past the 2048-block grid cap, so the grid-stride loop and the scalar tail both run
SZ = C.c_size_t


def check_folds(be, n):
    """mrs_resid_scale_add_f32: h * rs + y * 1 with three roundings (dec_epilogue.cuh resid_fold, -ffp-contract=off); mrs_vec_add_f32: a + b.  Both equal NumPy
    float32 bit for bit on [0, n) and leave the 8 elements after it alone."""
    rng = np.random.default_rng(n)
    h0, y0 = (rng.standard_normal(n + 8) * 3.0).astype(np.float32), rng.standard_normal(n + 8).astype(np.float32)
    fold, add = be.sym("mrs_resid_scale_add_f32", [VP, C.c_float, VP, SZ, VP], CI), be.sym("mrs_vec_add_f32", [VP, VP, SZ, VP], CI)
    y = be.buf(y0)
    for rs in (1.0, 0.5, 1.0 / 3.0):
        h = be.buf(h0)
        assert fold(h.ptr, rs, y.ptr, n, be.stream) == 0
        want = h0.copy()
        want[:n] = h0[:n] * np.float32(rs) + y0[:n] * np.float32(1.0)
        assert np.array_equal(h.numpy().view(np.uint32), want.view(np.uint32)), rs
    a = be.buf(h0)
    assert add(a.ptr, y.ptr, n, be.stream) == 0
    want = h0.copy()
    want[:n] = h0[:n] + y0[:n]
    assert np.array_equal(a.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(y.numpy().view(np.uint32), y0.view(np.uint32))


@pytest.mark.parametrize("n", FOLD_N)
def test_prompt_folds_host_emulation(n):
    check_folds(HostBackend(), n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", FOLD_N)
def test_prompt_folds_gpu(dev, n):
    check_folds(GpuBackend(dev), n)
