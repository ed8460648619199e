"""The grouped exact prompt GEMM of sparse-MoE prompts (csrc/ext_gemm_qi.hip; Llama::moe_ffn_exact in csrc/host/runtime.cpp) at window and tile edges, through the C ABI:
    mrs_gemm_qi_win     every row of an expert's window {begin, end} equals the decode engine's GEMV of that row (oracle gemv_engine) BIT FOR BIT, whatever tile of the
                        launch it falls in, and nothing outside the window is written;
    mrs_qi_gather_rows  the gathered operand image is byte-identical to quantizing the gathered rows directly, for both image layouts (Q8_K / Q8_0);
    mrs_moe_fold_exact  the slots fold into h in slot order, two roundings per slot (dec_epilogue.cuh resid_fold), restated in float32 NumPy;
    the composed step   quantize -> gather -> gate / up windows -> GLU quantize -> down windows -> fold with FORCED routing equals the per-token decode expression.
The routing tables are chosen, not routed: they put a window across a tile edge, start windows off every alignment, leave experts empty and make whole tiles lie past a
window's end (the workgroup tile is 128 tokens; the model-level prompts of tests/test_prefill_exact.py have 70).  Every comparison is exact: the references are the engine's
own stated order."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.abi_backends import GpuBackend, HostBackend

VP, CI, CF, LL = C.c_void_p, C.c_int, C.c_float, C.c_longlong
EPS = 1e-5


# ------------------------------------------------------------------------------------------------ routing tables
@functools.lru_cache(maxsize=None)
def routing(name):
    """-> (ids [T, tk] int32, E, the bounds launch_moe_dispatch must give)"""
    if name == "t150":  # an empty window at row 0; 128 + 22 rows; a window from row 150 with 129 rows (second tile: one row); 21 rows whose second tile must leave
        ids = np.empty((150, 2), np.int32)
        ids[:, 0] = 1
        ids[:129, 1] = 2
        ids[129:, 1] = 3
        return ids, 4, [0, 0, 150, 279, 300]
    if name == "t300":  # a one-row window, an empty one in the middle, 299 rows over three tiles from row 1
        ids = np.full((300, 1), 2, np.int32)
        ids[0, 0] = 0
        return ids, 3, [0, 1, 1, 300]
    if name == "t128":  # windows of exactly one tile, the second from row 128; an empty window at the end of the buffer
        ids = np.empty((128, 2), np.int32)
        ids[:, 0] = 0
        ids[:, 1] = 1
        return ids, 3, [0, 128, 256, 256]
    raise KeyError(name)


def dispatch(O, name):
    ids, E, expect = routing(name)
    T, tk = ids.shape
    bounds, order = O.moe_dispatch(ids, E, tk)[:2]
    assert bounds.tolist() == expect
    return ids, E, T, tk, np.ascontiguousarray(bounds, np.int32), np.ascontiguousarray(order, np.int32)


# ------------------------------------------------------------------------------------------------ launcher helpers
def repack_experts(O, be, t, packed, n, k):
    """E tensors of GGUF blocks -> one buffer of MFMA-order panels, expert e at e * mrs_gemm_qi_repack_bytes (as the runtime addresses them); -> (buffer, bytes per expert)"""
    nb = be.sym("mrs_gemm_qi_repack_bytes", [CI, LL, LL], C.c_size_t)(t, n, k)
    assert nb > 0 and nb % 16 == 0
    wq = be.buf(np.full(nb * len(packed), 0xA5, np.uint8))
    repack = be.sym("mrs_gemm_qi_repack", [VP, CI, LL, LL, VP, VP], CI)
    for e, p in enumerate(packed):
        src = be.buf(np.ascontiguousarray(p).reshape(-1))
        assert repack(src.ptr, t, n, k, wq.ptr + e * nb, be.stream) == 0
        src.numpy()  # the copy is done before `src` goes away
    return wq, nb


def act_bytes(be, rows, k):
    return be.sym("mrs_qi_act_bytes", [CI, CI], C.c_size_t)(rows, k)


def quantize_rows(be, t, x, k, norm_w=None, x2=None):
    """mrs_qi_quantize_for of the rows of x (x2: silu(x) * x2) into a zero-initialised image"""
    rows = x.shape[0]
    act = be.buf(np.zeros(act_bytes(be, rows, k), np.uint8))
    xb = be.buf(x)
    x2b = be.buf(x2) if x2 is not None else None
    nwb = be.buf(norm_w) if norm_w is not None else None
    tmp = be.buf(np.zeros((rows, k), np.float32)) if x2 is not None else None
    rc = be.sym("mrs_qi_quantize_for", [CI, VP, VP, CI, VP, CF, CI, CI, VP, VP, VP], CI)(t, xb.ptr, x2b.ptr if x2b else None, x.shape[1], nwb.ptr if nwb else None, EPS, rows, k, act.ptr,
                                                                                      tmp.ptr if tmp else None, be.stream)
    assert rc == 0, rc
    act.numpy()  # the image is complete before the inputs go away
    return act


@functools.lru_cache(maxsize=None)
def operand_rows(R, k):
    """R distinct random operand rows, the same for every weight type"""
    x = np.random.default_rng([R, k]).standard_normal((R, k)).astype(np.float32)
    x[2, :256] = 0.0  # an all-zero activation block
    x.setflags(write=False)
    return x


_HOST_IMAGES = {}


def operand_image(O, be, t, R, k):
    """the image of operand_rows(R, k) for weight type t.  The emulated Q8_K quantizer costs more than the GEMM it feeds, and the image depends on t only through its
    format (Q8_0 blocks / Q8_K), so the host emulation builds each (format, R, k) once and every case uploads a copy.  This leans on mrs_qi_quantize_for using w_type
    ONLY through dec2::act_mode_for (csrc/ext_gemm_qi.hip): if the quantizer ever looks at the type itself, key the cache by t.  The GPU cases quantize per type."""
    if not isinstance(be, HostBackend):
        return quantize_rows(be, t, operand_rows(R, k), k)
    key = (t == O.Q8_0, R, k)
    if key not in _HOST_IMAGES:
        _HOST_IMAGES[key] = quantize_rows(be, t, operand_rows(R, k), k).numpy().copy()
    return be.buf(_HOST_IMAGES[key])


def gemm_win(be):
    return be.sym("mrs_gemm_qi_win", [VP, CI, CI, CI, VP, CI, VP, CI, VP, CI, CI, VP], CI)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ A. mrs_gemm_qi_win
@functools.lru_cache(maxsize=None)
def win_reference(tname, route, n, k):
    """E expert tensors, R operand rows in expert-sorted order and the engine GEMV of every row by its window's expert: computed once, shared by both backends, read-only"""
    from oracle import oracle as O
    O.build()
    t = getattr(O, tname)
    ids, E, T, tk, bounds, order = dispatch(O, route)
    R = T * tk
    rng = np.random.default_rng([t, n, k, R])
    packed = [O.quantize(t, (rng.standard_normal((n, k)) * 0.05).astype(np.float32)).reshape(n, -1) for _ in range(E)]
    x = operand_rows(R, k)
    eng = np.empty((R, n), np.float32)
    for e in range(E):
        for r in range(bounds[e], bounds[e + 1]):
            eng[r] = O.gemv_engine(t, packed[e], n, k, x[r])[0]
    for a in packed + [x, eng]:
        a.setflags(write=False)
    return packed, x, eng


def check_win(O, be, tname, route, n, k, pad, acc):
    t = getattr(O, tname)
    ids, E, T, tk, bounds, order = dispatch(O, route)
    R, ldo = T * tk, n + pad
    packed, x, eng = win_reference(tname, route, n, k)
    wq, nb = repack_experts(O, be, t, packed, n, k)
    act = operand_image(O, be, t, R, k)
    bb = be.buf(bounds)
    rng = np.random.default_rng(R + n)
    base = rng.standard_normal((R, ldo)).astype(np.float32) if acc else np.full((R, ldo), np.nan, np.float32)
    ob = be.buf(base)
    fn = gemm_win(be)
    state = base.copy()  # what `out` must hold, bit for bit, after every launch
    for e in range(E):  # one launch per expert, max_rows = T as the runtime passes; after EACH launch only that expert's window may have changed
        assert fn(wq.ptr + e * nb, t, n, k, act.ptr, R, bb.ptr + 4 * e, T, ob.ptr, ldo, 1 if acc else 0, be.stream) == 0
        b0, b1 = int(bounds[e]), int(bounds[e + 1])
        state[b0:b1, :n] = base[b0:b1, :n] + eng[b0:b1] if acc else eng[b0:b1]
        got = ob.numpy()
        inside = np.zeros((R, ldo), bool)
        inside[b0:b1, :n] = True
        bad_out = (u32(got) != u32(state)) & ~inside
        assert not bad_out.any(), (tname, route, "expert", e, "wrote outside its window", np.argwhere(bad_out)[:4].tolist())
        assert np.array_equal(got[b0:b1, :n], state[b0:b1, :n]), (tname, route, "expert", e, "rows", (b0 + np.unique(np.argwhere(got[b0:b1, :n] != state[b0:b1, :n])[:, 0]))[:8].tolist())
    assert np.array_equal(u32(ob.numpy()), u32(state))


# (type, routing, N, K, ldo - N, accumulate): N = 160 -> two N tiles, the second partial, its last 32-row panel past N; K = 768 -> three superblocks (the double buffer wraps)
WIN_CASES = [("Q4_K", "t150", 160, 768, 4, 0), ("Q8_0", "t150", 160, 768, 4, 0), ("Q4_K", "t300", 160, 768, 0, 1), ("Q8_0", "t300", 160, 768, 0, 1),
             ("Q4_K", "t128", 160, 768, 4, 1), ("Q8_0", "t128", 160, 768, 0, 0), ("Q5_K", "t150", 160, 768, 4, 1), ("Q6_K", "t300", 160, 768, 4, 0),
             ("Q5_K", "t300", 40, 512, 0, 0), ("Q6_K", "t150", 40, 512, 0, 1), ("Q4_K", "t150", 40, 512, 0, 1), ("Q8_0", "t300", 40, 512, 4, 1)]


@pytest.mark.parametrize("tname,route,n,k,pad,acc", WIN_CASES)
def test_gemm_qi_win_host_emulation(oracle, tname, route, n, k, pad, acc):
    check_win(oracle, HostBackend(), tname, route, n, k, pad, acc)


@pytest.mark.gpu
@pytest.mark.parametrize("tname,route,n,k,pad,acc", WIN_CASES)
def test_gemm_qi_win_gpu(oracle, dev, tname, route, n, k, pad, acc):
    check_win(oracle, GpuBackend(dev), tname, route, n, k, pad, acc)


@pytest.mark.parametrize("tname", ["Q4_K", "Q8_0"])
def test_gemm_qi_win_refusals_host_emulation(oracle, tname):
    """no window, no rows, more rows than the operand buffer holds: -1, nothing written"""
    be, t, n, k, R = HostBackend(), getattr(oracle, tname), 40, 512, 6
    rng = np.random.default_rng(3)
    wq, nb = repack_experts(oracle, be, t, [oracle.quantize(t, (rng.standard_normal((n, k)) * 0.05).astype(np.float32))], n, k)
    act = quantize_rows(be, t, rng.standard_normal((R, k)).astype(np.float32), k)
    bb = be.buf(np.array([0, R], np.int32))
    base = rng.standard_normal((R, n)).astype(np.float32)
    ob = be.buf(base)
    fn = gemm_win(be)
    for win, max_rows in ((None, R), (bb.ptr, 0), (bb.ptr, R + 1)):
        assert fn(wq.ptr, t, n, k, act.ptr, R, win, max_rows, ob.ptr, n, 0, be.stream) == -1
        assert np.array_equal(u32(ob.numpy()), u32(base))
    assert fn(wq.ptr, t, n, k, act.ptr, R, bb.ptr, R, ob.ptr, n, 0, be.stream) == 0  # the same arguments with a window and rows: taken
    assert not np.array_equal(u32(ob.numpy()), u32(base))


# ------------------------------------------------------------------------------------------------ B. mrs_qi_gather_rows
def gather_fn(be):
    return be.sym("mrs_qi_gather_rows", [CI, VP, CI, VP, CI, CI, VP, CI, VP, VP], CI)


def check_gather(O, be, tname, k):
    t = getattr(O, tname)
    ids, E, T, tk, bounds, order = dispatch(O, "t150")  # T = 150: no multiple of 4
    R = T * tk
    rng = np.random.default_rng(k + t)
    x = rng.standard_normal((T, k)).astype(np.float32)
    x[1, :256] = 0.0
    src = quantize_rows(be, t, x, k)
    want = quantize_rows(be, t, np.ascontiguousarray(x[order // tk]), k).numpy()
    sb = be.buf(order)
    fn = gather_fn(be)
    dst, inv = be.buf(np.zeros(act_bytes(be, R, k), np.uint8)), be.buf(np.full(R, -7, np.int32))
    assert fn(t, src.ptr, T, dst.ptr, R, k, sb.ptr, tk, inv.ptr, be.stream) == 0
    got = dst.numpy()
    assert got.shape == want.shape and np.array_equal(got, want), (tname, k, int((got != want).sum()), np.flatnonzero(got != want)[:4].tolist())
    iv = inv.numpy()
    assert np.array_equal(iv[order], np.arange(R)), "inv[sorted[r]] != r"
    dst2 = be.buf(np.zeros(act_bytes(be, R, k), np.uint8))
    assert fn(t, src.ptr, T, dst2.ptr, R, k, sb.ptr, tk, None, be.stream) == 0  # inv = NULL is accepted
    assert np.array_equal(dst2.numpy(), want)
    # refusals return before any launch
    assert fn(t, src.ptr, T, dst.ptr, R, k + 44, sb.ptr, tk, inv.ptr, be.stream) == -1
    assert fn(t, src.ptr, T, dst.ptr, R, k, sb.ptr, 0, inv.ptr, be.stream) == -1
    assert fn(O.Q4_0, src.ptr, T, dst.ptr, R, k, sb.ptr, tk, inv.ptr, be.stream) == -1
    assert np.array_equal(dst.numpy(), want) and np.array_equal(inv.numpy(), iv)


GATHER_CASES = [("Q4_K", 256), ("Q4_K", 768), ("Q8_0", 256), ("Q8_0", 768)]


@pytest.mark.parametrize("tname,k", GATHER_CASES)
def test_qi_gather_rows_host_emulation(oracle, tname, k):
    check_gather(oracle, HostBackend(), tname, k)


@pytest.mark.gpu
@pytest.mark.parametrize("tname,k", GATHER_CASES)
def test_qi_gather_rows_gpu(oracle, dev, tname, k):
    check_gather(oracle, GpuBackend(dev), tname, k)


# ------------------------------------------------------------------------------------------------ C. mrs_moe_fold_exact
def fold_fn(be):
    return be.sym("mrs_moe_fold_exact", [VP, CF, VP, VP, VP, CI, CI, CI, VP], CI)


def fold_reference(h, rs, y, inv, w, T, tk):
    """dec::resid_fold over the slots in order: old * (sl == 0 ? rs : 1) + y * w, every product and every sum rounded to f32"""
    want = h.copy()
    for sl in range(tk):
        sc = np.float32(rs if sl == 0 else 1.0)
        want[:T] = (want[:T] * sc).astype(np.float32) + (y[inv[np.arange(T) * tk + sl]] * w[:, sl:sl + 1]).astype(np.float32)
    return want


def check_fold(be, d):
    T = 5
    fn = fold_fn(be)
    for tk in (1, 2, 3):
        R = T * tk
        rng = np.random.default_rng(d + tk)
        h0 = (rng.standard_normal((T + 2, d)) * 3.0).astype(np.float32)  # two rows more than T: they keep their bits
        y0 = rng.standard_normal((R, d)).astype(np.float32)
        inv0 = rng.permutation(R).astype(np.int32)
        w0 = rng.uniform(0.05, 1.0, (T, tk)).astype(np.float32)
        y, inv, w = be.buf(y0), be.buf(inv0), be.buf(w0)
        for rs in (1.0, 0.5):
            h = be.buf(h0)
            assert fn(h.ptr, rs, y.ptr, inv.ptr, w.ptr, T, d, tk, be.stream) == 0
            want = fold_reference(h0, rs, y0, inv0, w0, T, tk)
            assert np.array_equal(u32(h.numpy()), u32(want)), (d, tk, rs, int((u32(h.numpy()) != u32(want)).sum()))
        assert np.array_equal(u32(y.numpy()), u32(y0))
    h = be.buf(h0)
    assert fn(h.ptr, 1.0, y.ptr, inv.ptr, w.ptr, T, d + 2, 3, be.stream) == -1  # d % 4 != 0: refused before any launch
    assert np.array_equal(u32(h.numpy()), u32(h0))


FOLD_D = [4, 516, 1028]  # below one pass of the 256 threads, a partial pass, past the 1024-column stride


@pytest.mark.parametrize("d", FOLD_D)
def test_moe_fold_exact_host_emulation(d):
    check_fold(HostBackend(), d)


@pytest.mark.gpu
@pytest.mark.parametrize("d", FOLD_D)
def test_moe_fold_exact_gpu(dev, d):
    check_fold(GpuBackend(dev), d)


# ------------------------------------------------------------------------------------------------ D. the composed step with forced routing
RS_STEP = 0.5  # the residual scale of a two-rank tensor-parallel layer: the first slot's scale differs from the others'


@functools.lru_cache(maxsize=None)
def step_reference(tg_name, td_name, d, ff):
    """per token and slot in order: a = glu(gate_e . xn, up_e . xn); h <- h * (sl == 0 ? rs : 1) + (down_e . a) * w -- the decode step of a sparse-MoE layer"""
    from oracle import oracle as O
    O.build()
    tg, td = getattr(O, tg_name), getattr(O, td_name)
    ids, E, T, tk, bounds, order = dispatch(O, "t150")
    rng = np.random.default_rng([tg, td, d, ff])
    q = lambda t, n, k: O.quantize(t, (rng.standard_normal((n, k)) * 0.05).astype(np.float32)).reshape(n, -1)
    gate, up, down = [q(tg, ff, d) for _ in range(E)], [q(tg, ff, d) for _ in range(E)], [q(td, d, ff) for _ in range(E)]
    h0 = rng.standard_normal((T, d)).astype(np.float32)
    nw = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    w = rng.uniform(0.05, 1.0, (T, tk)).astype(np.float32)
    xn = O.rms_norm_engine(h0, nw, EPS)
    want = h0.copy()
    for tok in range(T):
        for sl in range(tk):
            e = int(ids[tok, sl])
            a = O.fused_glu_engine(O.gemv_engine(tg, gate[e], ff, d, xn[tok]), O.gemv_engine(tg, up[e], ff, d, xn[tok]))
            s = O.gemv_engine(td, down[e], d, ff, a)[0]
            want[tok] = (want[tok] * np.float32(RS_STEP if sl == 0 else 1.0)).astype(np.float32) + (s * w[tok, sl]).astype(np.float32)
    for a in gate + up + down + [h0, nw, w, want]:
        a.setflags(write=False)
    return gate, up, down, h0, nw, w, want


def check_step(O, be, tg_name, td_name, d=512, ff=768):
    tg, td = getattr(O, tg_name), getattr(O, td_name)
    ids, E, T, tk, bounds, order = dispatch(O, "t150")
    R = T * tk
    gate, up, down, h0, nw, w, want = step_reference(tg_name, td_name, d, ff)
    gq, pg = repack_experts(O, be, tg, gate, ff, d)
    uq, _ = repack_experts(O, be, tg, up, ff, d)
    dq, pd = repack_experts(O, be, td, down, d, ff)
    bb, sb, inv, wb = be.buf(bounds), be.buf(order), be.buf(np.full(R, -7, np.int32)), be.buf(w)
    h = be.buf(h0)
    qact = quantize_rows(be, tg, h0, d, norm_w=nw)
    qact_g = be.buf(np.zeros(act_bytes(be, R, d), np.uint8))
    assert gather_fn(be)(tg, qact.ptr, T, qact_g.ptr, R, d, sb.ptr, tk, inv.ptr, be.stream) == 0
    rg, ru, y = be.buf(np.full((R, ff), np.nan, np.float32)), be.buf(np.full((R, ff), np.nan, np.float32)), be.buf(np.full((R, d), np.nan, np.float32))
    fn = gemm_win(be)
    for e in range(E):
        assert fn(gq.ptr + e * pg, tg, ff, d, qact_g.ptr, R, bb.ptr + 4 * e, T, rg.ptr, ff, 0, be.stream) == 0
        assert fn(uq.ptr + e * pg, tg, ff, d, qact_g.ptr, R, bb.ptr + 4 * e, T, ru.ptr, ff, 0, be.stream) == 0
    qact_r, ract = be.buf(np.zeros(act_bytes(be, R, ff), np.uint8)), be.buf(np.zeros((R, ff), np.float32))
    assert be.sym("mrs_qi_quantize_for", [CI, VP, VP, CI, VP, CF, CI, CI, VP, VP, VP], CI)(td, rg.ptr, ru.ptr, ff, None, 0.0, R, ff, qact_r.ptr, ract.ptr, be.stream) == 0
    for e in range(E):
        assert fn(dq.ptr + e * pd, td, d, ff, qact_r.ptr, R, bb.ptr + 4 * e, T, y.ptr, d, 0, be.stream) == 0
    assert fold_fn(be)(h.ptr, RS_STEP, y.ptr, inv.ptr, wb.ptr, T, d, tk, be.stream) == 0
    got = h.numpy()
    assert np.array_equal(got, want), (tg_name, td_name, "tokens", np.unique(np.argwhere(got != want)[:, 0])[:8].tolist())


STEP_CASES = [("Q4_K", "Q6_K"), ("Q8_0", "Q8_0")]


@pytest.mark.parametrize("tg,td", STEP_CASES)
def test_moe_exact_step_forced_routing_host_emulation(oracle, tg, td):
    check_step(oracle, HostBackend(), tg, td)


@pytest.mark.gpu
@pytest.mark.parametrize("tg,td", STEP_CASES)
def test_moe_exact_step_forced_routing_gpu(oracle, dev, tg, td):
    check_step(oracle, GpuBackend(dev), tg, td)
