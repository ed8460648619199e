"""GPU parity: RoPE, fused GLU, RMSNorm family vs the oracle.
Bars: f32 -> <= 2 ulp-ish (rsqrt / exp approximations: 1e-6 relative); f16/bf16 -> the reference
rounds after every arithmetic step, reproduced in the expected value; <= 1 storage ulp allowed."""
import numpy as np
import pytest

from tests.util import round_through, to_np, torch_dtype

pytestmark = pytest.mark.gpu
ULP = {"f32": 2.0 ** -23, "f16": 2.0 ** -10, "bf16": 2.0 ** -7}


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("neox", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
def test_rotary(oracle, dev, dt, neox, with_pos):
    import torch
    from mistralrs_amd import ops
    rng = np.random.default_rng(3)
    T, H, KVH, hd, maxpos = 7, 8, 2, 128, 64
    inv = 1.0 / (500000.0 ** (np.arange(0, hd, 2) / hd))
    ang = np.arange(maxpos)[:, None] * inv[None, :]
    cos, sin = round_through(np.cos(ang).astype(np.float32), dt), round_through(np.sin(ang).astype(np.float32), dt)
    q = round_through(rng.standard_normal((T, H, hd)).astype(np.float32), dt)
    k = round_through(rng.standard_normal((T, KVH, hd)).astype(np.float32), dt)
    pos = rng.integers(0, maxpos, T).astype(np.int32) if with_pos else np.arange(T, dtype=np.int32)
    td = torch_dtype(dt)
    qt, kt = torch.from_numpy(q).to(dev).to(td), torch.from_numpy(k).to(dev).to(td)
    ops.apply_rotary_qk(qt, kt, torch.from_numpy(cos).to(dev).to(td), torch.from_numpy(sin).to(dev).to(td), neox,
                        torch.from_numpy(pos).to(dev) if with_pos else None)
    for got, x in ((to_np(qt), q), (to_np(kt), k)):
        want = oracle.rope(x, cos, sin, pos, neox)
        tol = 3 * ULP[dt] * (np.abs(x).max() * 2)  # each product and the sum round once in dt
        assert np.abs(got - want).max() <= tol + 1e-6
        if dt != "f32":  # exact: the per-operation rounding of the reference's 16-bit instantiation (pinned in tests/test_oracle_ref.py)
            from tests.test_oracle_ref import _rope16
            np.testing.assert_array_equal(got, _rope16(x, cos, sin, pos, neox, dt))


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_fused_glu_op(oracle, dev, dt, act):
    import torch
    from mistralrs_amd import ops
    rng = np.random.default_rng(act)
    wide = round_through(rng.standard_normal((5, 2 * 1001)).astype(np.float32) * 3, dt)
    wt = torch.from_numpy(wide).to(dev).to(torch_dtype(dt))
    a, b = wt[:, :1001], wt[:, 1001:]  # strided rows, odd width -> scalar path
    got = to_np(ops.fused_glu(a, b, act))
    want = round_through(round_through(oracle.fused_glu(wide[:, :1001], np.ones((5, 1001), np.float32), act), dt) * wide[:, 1001:], dt)
    tol = 2 * ULP[dt] * np.abs(want) + 2e-6 * np.abs(wide[:, 1001:]) * (np.abs(wide[:, :1001]) + 1)
    assert (np.abs(got - want) <= tol + 1e-30).all()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("rows,cols", [(3, 4096), (2, 1000), (1, 14336), (2, 20000)])
def test_rms_norm_family(oracle, dev, dt, rows, cols):
    import torch
    from mistralrs_amd import ops
    rng = np.random.default_rng(cols)
    td = torch_dtype(dt)
    x = round_through(rng.standard_normal((rows, cols)).astype(np.float32), dt)
    r = round_through(rng.standard_normal((rows, cols)).astype(np.float32), dt)
    w = round_through(1 + 0.1 * rng.standard_normal(cols).astype(np.float32), dt)
    xt, rt, wt = (torch.from_numpy(a).to(dev).to(td) for a in (x, r, w))
    eps = 1e-5
    tol = lambda want: 1.01 * ULP[dt] * np.abs(want) + 4e-6 * np.abs(want) + 1e-7
    want = oracle.rms_norm(x, w, eps)
    got = to_np(ops.rms_norm(xt, wt, eps))
    assert (np.abs(got - (round_through(want, dt) if dt != "f32" else want)) <= tol(want)).all()
    # add_rms_norm: residual_out = T(x + r) exactly; norm over the ROUNDED sum (sort.cu:403-428)
    res, nrm = ops.add_rms_norm(xt, rt, wt, eps)
    s = round_through(x + r, dt)
    np.testing.assert_array_equal(to_np(res), s)
    want = oracle.rms_norm(s, w, eps)
    assert (np.abs(to_np(nrm) - (round_through(want, dt) if dt != "f32" else want)) <= tol(want)).all()
    # rms_norm_residual: (r + rms(x)*w) * scale
    sc = round_through(np.array([0.5], np.float32), dt)
    got = to_np(ops.rms_norm_residual(xt, rt, wt, eps, torch.from_numpy(sc).to(dev).to(td)))
    want = (r + oracle.rms_norm(x, w, eps)) * sc[0]
    assert (np.abs(got - (round_through(want, dt) if dt != "f32" else want)) <= tol(want) + 4e-6 * np.abs(r)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# Paths the cases above never reach: the scalar RMSNorm kernel (odd widths, misaligned pointers), partial rotary / several loop
# trips / strided q,k in RoPE, the grid-stride loop / unequal row strides / saturating activations of fused_glu.
def _check_rms_family(oracle, dt, x, r, w, xt, rt, wt, eps=1e-5):
    """The three ops on one (x, residual, weight) triple with the bars of test_rms_norm_family, plus rms_norm_residual(scale=None)."""
    import torch
    from mistralrs_amd import ops
    td = torch_dtype(dt)
    rnd = lambda a: round_through(a, dt) if dt != "f32" else a
    tol = lambda want: 1.01 * ULP[dt] * np.abs(want) + 4e-6 * np.abs(want) + 1e-7
    want = oracle.rms_norm(x, w, eps)
    got = to_np(ops.rms_norm(xt, wt, eps))
    assert got.shape == x.shape and (np.abs(got - rnd(want)) <= tol(want)).all()
    res, nrm = ops.add_rms_norm(xt, rt, wt, eps)
    s = round_through(x + r, dt)
    np.testing.assert_array_equal(to_np(res), s)
    want = oracle.rms_norm(s, w, eps)
    assert (np.abs(to_np(nrm) - rnd(want)) <= tol(want)).all()
    sc = round_through(np.array([0.5], np.float32), dt)
    got = to_np(ops.rms_norm_residual(xt, rt, wt, eps, torch.from_numpy(sc).to(xt.device).to(td)))
    want = (r + oracle.rms_norm(x, w, eps)) * sc[0]
    assert (np.abs(got - rnd(want)) <= tol(want) + 4e-6 * np.abs(r)).all()
    got = to_np(ops.rms_norm_residual(xt, rt, wt, eps, None))  # null scale pointer: (r + rms(x) * w)
    want = r + oracle.rms_norm(x, w, eps)
    assert (np.abs(got - rnd(want)) <= tol(want) + 4e-6 * np.abs(r)).all()


def _rms_inputs(dt, rows, cols, seed):
    rng = np.random.default_rng(seed)
    x = round_through(rng.standard_normal((rows, cols)).astype(np.float32), dt)
    r = round_through(rng.standard_normal((rows, cols)).astype(np.float32), dt)
    w = round_through(1 + 0.1 * rng.standard_normal(cols).astype(np.float32), dt)
    return x, r, w


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("rows,cols", [(3, 1001), (2, 7), (1, 1), (2, 4100), (2, 4101)])
def test_rms_norm_family_scalar_widths(oracle, dev, dt, rows, cols):
    """Widths that are no multiple of the 16-byte vector (4 f32 / 8 f16,bf16 elements) take rms_norm_kernel<T, MODE, false>: several trips of
    its 256-thread loop with idle threads in the last (1001, 4100, 4101), fewer columns than one vector (7, 1).  4100 is a vector multiple for
    f32 only (there it is one more vector-path width), 4101 is scalar for every dtype."""
    import torch
    x, r, w = _rms_inputs(dt, rows, cols, cols)
    xt, rt, wt = (torch.from_numpy(a).to(dev).to(torch_dtype(dt)) for a in (x, r, w))
    _check_rms_family(oracle, dt, x, r, w, xt, rt, wt)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("which", ["none", "all", "weight"])
def test_rms_norm_family_misaligned_base(oracle, dev, dt, which):
    """A vector-multiple width whose pointers are not 16-byte aligned must take the scalar kernel (launch_rms: `al % 16 == 0`): x, residual and
    weight are contiguous views one element into a larger buffer ("all"), or only the weight is ("weight"); "none" is the aligned vector
    path of the same shape for the scale=None branch."""
    import torch
    rows, cols = 2, 1024
    x, r, w = _rms_inputs(dt, rows, cols, 77)
    td = torch_dtype(dt)

    def place(a, shifted):
        if not shifted:
            t = torch.from_numpy(a).to(dev).to(td)
            assert t.data_ptr() % 16 == 0
            return t
        buf = torch.zeros(a.size + 8, dtype=td, device=dev)
        view = buf[1:1 + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a).to(dev).to(td))
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view
    xt, rt, wt = place(x, which == "all"), place(r, which == "all"), place(w, which != "none")
    _check_rms_family(oracle, dt, x, r, w, xt, rt, wt)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("cols", [1024, 1001])
def test_rms_norm_family_zero_row(oracle, dev, dt, cols):
    """A row of zeros has sum of squares 0, so inv = rsqrt(eps) is finite and the row normalises to exactly 0: rms_norm and add_rms_norm give 0,
    rms_norm_residual gives residual * scale (0.5: exact).  The other row keeps the usual bars."""
    import torch
    from mistralrs_amd import ops
    x, r, w = _rms_inputs(dt, 2, cols, cols + 1)
    x[0] = 0.0
    td = torch_dtype(dt)
    xt, rt, wt = (torch.from_numpy(a).to(dev).to(td) for a in (x, r, w))
    _check_rms_family(oracle, dt, x, r, w, xt, rt, wt)
    eps = 1e-5
    got = to_np(ops.rms_norm(xt, wt, eps))
    assert np.isfinite(got).all() and (got[0] == 0).all()
    r0 = r.copy()
    r0[0] = 0.0
    res, nrm = ops.add_rms_norm(xt, torch.from_numpy(r0).to(dev).to(td), wt, eps)
    assert np.isfinite(to_np(nrm)).all() and (to_np(res)[0] == 0).all() and (to_np(nrm)[0] == 0).all()
    sc = torch.from_numpy(np.array([0.5], np.float32)).to(dev).to(td)
    got = to_np(ops.rms_norm_residual(xt, rt, wt, eps, sc))
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[0], round_through(r[0] * np.float32(0.5), dt))


# (tokens, heads, kv_heads, head_size, rotated pairs): partial rotary at two head sizes; 2048 / 512 work items (four trips of the 512-thread loop for q, one
# full trip for k); 24 items in a 64-thread block; 120 items in a block rounded up to 128
ROPE_SHAPES = [(7, 8, 2, 128, 32), (3, 4, 2, 96, 16), (2, 32, 8, 128, 64), (1, 1, 1, 64, 24), (5, 3, 3, 80, 40)]


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("neox", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("T,H,KVH,hd,pairs", ROPE_SHAPES)
def test_rotary_partial_strided_and_loop_trips(oracle, dev, dt, neox, with_pos, T, H, KVH, hd, pairs):
    """q and k are the first two parts of one fused [q | k | v] row (token stride > heads * head_size).  Same bars as test_rotary; in addition every
    element past the rotated width and the whole v part keep their bits."""
    import torch
    from mistralrs_amd import ops
    from tests.test_oracle_ref import _rope16
    rng = np.random.default_rng(T * 1000 + hd + pairs)
    maxpos = 64
    inv = 1.0 / (500000.0 ** (np.arange(0, 2 * pairs, 2) / (2 * pairs)))
    ang = np.arange(maxpos)[:, None] * inv[None, :]
    cos, sin = round_through(np.cos(ang).astype(np.float32), dt), round_through(np.sin(ang).astype(np.float32), dt)
    nq, nk = H * hd, KVH * hd
    wide = round_through(rng.standard_normal((T, nq + 2 * nk)).astype(np.float32), dt)
    q, k = wide[:, :nq].reshape(T, H, hd), wide[:, nq:nq + nk].reshape(T, KVH, hd)
    # rows 0 and maxpos - 1, repeats; int32 on the device (the kernel reads them as uint32)
    pos = np.array([maxpos - 1, 0, maxpos - 1, 7, 0, 13, 7], dtype=np.int32)[:T] if with_pos else np.arange(T, dtype=np.int32)
    td = torch_dtype(dt)
    wt = torch.from_numpy(wide).to(dev).to(td)
    qt, kt = wt[:, :nq].view(T, H, hd), wt[:, nq:nq + nk].view(T, KVH, hd)
    assert T == 1 or (qt.stride(0) == nq + 2 * nk and kt.stride(0) == nq + 2 * nk)  # one token: the stride of a size-1 dimension is never used
    assert qt.data_ptr() == wt.data_ptr()
    post = torch.from_numpy(pos).to(dev)
    assert post.dtype == torch.int32
    ops.apply_rotary_qk(qt, kt, torch.from_numpy(cos).to(dev).to(td), torch.from_numpy(sin).to(dev).to(td), neox, post if with_pos else None)
    after = to_np(wt)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    for got, x in ((after[:, :nq].reshape(T, H, hd), q), (after[:, nq:nq + nk].reshape(T, KVH, hd), k)):
        want = oracle.rope(x, cos, sin, pos, neox)
        tol = 3 * ULP[dt] * (np.abs(x).max() * 2)  # each product and the sum round once in dt
        assert np.abs(got - want).max() <= tol + 1e-6
        if dt != "f32":
            np.testing.assert_array_equal(got, _rope16(x, cos, sin, pos, neox, dt))
        np.testing.assert_array_equal(bits(got[..., 2 * pairs:]), bits(x[..., 2 * pairs:]))
    np.testing.assert_array_equal(bits(after[:, nq + nk:]), bits(wide[:, nq + nk:]))


def _glu_check(oracle, dt, act, a_np, b_np, got):
    """The bar of test_fused_glu_op: T(T(act(a)) * b) within 2 storage ulp + the f32 activation error."""
    with np.errstate(over="ignore"):  # test_fused_glu_saturation multiplies the largest finite value by -3 on purpose
        want = round_through(round_through(oracle.fused_glu(a_np, np.ones_like(a_np), act), dt) * b_np, dt)
        tol = 2 * ULP[dt] * np.abs(want) + 2e-6 * np.abs(b_np) * (np.abs(a_np) + 1)
    return want, tol


@pytest.mark.parametrize("dt", ["bf16"])
def test_fused_glu_grid_stride(oracle, dev, dt):
    """40 x 14336 = 573440 elements > 2048 blocks * 256 threads: the launch is capped and every thread of the first 49152 takes a second trip.
    bf16 + silu only: the loop depends on neither, and on the CPU emulation this one case costs more than the rest of the file."""
    import torch
    from mistralrs_amd import ops
    act, rows, cols = 0, 40, 14336
    assert rows * cols > 2048 * 256
    rng = np.random.default_rng(11)
    wide = round_through(rng.standard_normal((rows, 2 * cols)).astype(np.float32) * 3, dt)
    wt = torch.from_numpy(wide).to(dev).to(torch_dtype(dt))
    got = to_np(ops.fused_glu(wt[:, :cols], wt[:, cols:], act))
    want, tol = _glu_check(oracle, dt, act, wide[:, :cols], wide[:, cols:], got)
    assert (np.abs(got - want) <= tol + 1e-30).all()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("cols", [1001, 1024])
def test_fused_glu_unequal_row_strides(oracle, dev, dt, act, cols):
    """a and b are column windows of two tensors of different width, so a.stride(0) != b.stride(0)."""
    import torch
    from mistralrs_amd import ops
    rng = np.random.default_rng(cols + act)
    wa = round_through(rng.standard_normal((5, cols + 24)).astype(np.float32) * 3, dt)
    wb = round_through(rng.standard_normal((5, 2 * cols + 8)).astype(np.float32) * 3, dt)
    wat, wbt = (torch.from_numpy(t).to(dev).to(torch_dtype(dt)) for t in (wa, wb))
    a, b = wat[:, 8:8 + cols], wbt[:, cols:2 * cols]
    assert a.stride(0) != b.stride(0) and a.stride(0) != cols and b.stride(0) != cols
    got = to_np(ops.fused_glu(a, b, act))
    want, tol = _glu_check(oracle, dt, act, wa[:, 8:8 + cols], wb[:, cols:2 * cols], got)
    assert (np.abs(got - want) <= tol + 1e-30).all()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_fused_glu_saturation(oracle, dev, dt, act):
    """Arguments at which expf / tanhf / erff saturate, underflow or overflow, up to the dtype's largest finite value, against b = 1 and b = -3.
    Every result is finite and within the bar of test_fused_glu_op, with one exception that belongs to the operation and not to the kernel: for
    a = +-max the identity-like activations return +-max itself, and max * -3 is not representable.  There the oracle overflows as well, and the
    kernel must give the same signed infinity."""
    import torch
    from mistralrs_amd import ops
    big = {"f32": np.finfo(np.float32).max, "f16": np.float32(65504.0), "bf16": np.float32(2.0 ** 127 * (2 - 2.0 ** -7))}[dt]
    mags = np.array([0.0, 1e-4, 20.0, 88.0, 100.0, 1e4, big], dtype=np.float32)
    row = round_through(np.stack([mags, -mags], axis=1).reshape(-1), dt)
    assert np.isfinite(row).all() and row[-2] == big and np.signbit(row[1]) and row[1] == 0
    a_np = np.stack([row, row])
    b_np = np.stack([np.full_like(row, 1.0), np.full_like(row, -3.0)])
    td = torch_dtype(dt)
    got = to_np(ops.fused_glu(torch.from_numpy(a_np).to(dev).to(td), torch.from_numpy(b_np).to(dev).to(td), act))
    want, tol = _glu_check(oracle, dt, act, a_np, b_np, got)
    fin = np.isfinite(want)
    assert fin[0].all() and fin[1, :-2].all()          # b = 1 never overflows; b = -3 only at a = +-max
    assert not np.isnan(got).any() and (np.isfinite(got) == fin).all()
    np.testing.assert_array_equal(got[~fin], want[~fin])
    assert (np.abs(got[fin] - want[fin]) <= tol[fin] + 1e-30).all()
