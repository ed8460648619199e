"""FP8 (E4M3) KV pages in the decode engine and the exact prompt path, kernel level (csrc/dec_epilogue.cuh qkv_store_f8, csrc/dec_attn.cuh AttnRegs / unpack_f8_scaled,
the *_f8 entry points of include/mrs_hip_ext.h).  Every comparison is bit for bit:
  1. page writes      codes == fp8_e4m3_encode(rope(gemv_engine(rms_norm_engine(x))) / scale) from the oracle, for every producer kernel;
  2. decode attention == oracle.attention_engine on f32(decode(code) * scale), NaN codes in every slot the kernel must not use;
  3. prompt attention row t == decode attention at context start + t + 1 (matrix-core kernel and the vector-ALU fallback);
  4. the codec on the device: all 256 codes through a page.
Same bodies on the wave64 host emulation (CPU suite) and on the MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

from tests.abi_backends import GpuBackend, HostBackend
from tests.test_dec_engine import ATTN2, PROJ, PROJ_IMG, Mat, _act_image, _weights, repack
from tests.test_dec_mm import qi_repack
from tests.test_prefill_exact import PA

VP, CI, CF = C.c_void_p, C.c_int, C.c_float
QKV_F8 = [C.POINTER(Mat)] * 3 + [VP, CI, VP, CF] + [VP] * 7 + [CI] * 5 + [CF, CF, VP]
QKV_IMG_F8 = [C.POINTER(Mat)] * 3 + [VP] * 8 + [CI] * 6 + [CF, CF, VP]
MM_QKV_F8 = [VP, CI, CI] * 3 + [CI, VP] + [VP] * 7 + [CI] * 5 + [CF, CF, VP]
ATTN_F8 = [VP] * 9 + [CI, CF, VP, VP] + [CI] * 10 + [CF, CF, VP]
PA_F8 = [VP] * 6 + [CI] * 8 + [CF, CI, CI, CI, CF, CF, VP]
KS, VS = 0.037, 0.11  # not powers of two: the division's rounding counts
NAN = 0x7F


def _wide_range_weights(O, t, n, k, seed):
    """Quantized [n][k] weights whose outputs span the whole E4M3 range once divided by the scales: every row lives in ONE half of the reduction (the norm weights of the
    second half are 1e-4 of the first, _norm_w) and carries its own factor 10^-u, u in [0, 2.5]."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    w *= (10.0 ** -rng.uniform(0.0, 2.5, n)).astype(np.float32)[:, None]
    second = rng.random(n) < 0.5
    w[second, : k // 2] = 0.0
    w[~second, k // 2:] = 0.0
    return O.quantize(t, w).reshape(n, -1)


def _norm_w(k, rng):
    nw = (40.0 * (1.0 + 0.05 * rng.standard_normal(k))).astype(np.float32)
    nw[k // 2:] *= np.float32(1e-4)
    return nw


def _assert_codes_cover_the_format(codes):
    """on the oracle's expected codes alone: a saturated code of each sign, a subnormal, +0 and -0"""
    c = np.asarray(codes, np.uint8).reshape(-1)
    assert (c == 0x7E).any() and (c == 0xFE).any(), "no saturated code of each sign"
    assert (((c >> 3) & 15 == 0) & ((c & 7) != 0)).any(), "no subnormal code"
    assert (c == 0x00).any() and (c == 0x80).any(), "no +0 / -0"


def check_page_writes(O, be, tq, tv, heads, kvh, k, b, route):
    """route: 'inline' (mrs_dec_qkv_f8), 'neox' (mrs_dec_qkv_neox_f8), 'img' / 'img-neox' (mrs_dec_qkv_img_f8), 'mm' (mrs_dec_mm_qkv_f8)"""
    hd, bs = 128, 32
    nq, nkv = heads * hd, kvh * hd
    Tq, Tv = getattr(O, tq), getattr(O, tv)
    neox = route in ("neox", "img-neox")
    pq, pk, pv = _wide_range_weights(O, Tq, nq, k, 21), _wide_range_weights(O, Tq, nkv, k, 22), _wide_range_weights(O, Tv, nkv, k, 23)
    order = np.stack([np.arange(hd // 2), np.arange(hd // 2) + hd // 2], axis=1).reshape(-1)  # pair order of the rotate-half planes
    perm = (lambda p, h: p.reshape(h, hd, -1)[:, order].reshape(h * hd, -1)) if neox else (lambda p, h: p)
    kq, mq = repack(be, O, Tq, perm(pq, heads), nq, k)
    kk, mk = repack(be, O, Tq, perm(pk, kvh), nkv, k)
    kv, mv = repack(be, O, Tv, pv, nkv, k)
    rng = np.random.default_rng(24 + b)
    x = rng.standard_normal((b, k)).astype(np.float32)
    nw = _norm_w(k, rng)
    inv = 1.0 / (10000.0 ** (np.arange(0, hd, 2, dtype=np.float32) / hd))
    fr = np.arange(64, dtype=np.float32)[:, None] * inv[None, :]
    cos, sin = np.cos(fr).astype(np.float32), np.sin(fr).astype(np.float32)
    pos = np.array([5 + 7 * i for i in range(b)], dtype=np.int32)
    slots = np.array([(2 * i) * bs + int(pos[i]) % bs for i in range(b)], dtype=np.int64)
    if b > 1:
        slots[b - 1] = -1  # a padded sequence: nothing is written for it
    # the oracle's pages
    xn = O.rms_norm_engine(x, nw, 1e-5)
    lin = lambda t, p, n: np.concatenate([O.gemv_engine(t, p, n, k, r) for r in xn], axis=0)
    q_want = O.rope(lin(Tq, pq, nq).reshape(b, heads, hd), cos, sin, pos, neox).reshape(b, nq)
    k_want = O.rope(lin(Tq, pk, nkv).reshape(b, kvh, hd), cos, sin, pos, neox).reshape(b, nkv)
    v_want = lin(Tv, pv, nkv)
    k_codes, v_codes = O.fp8_e4m3_encode(k_want / np.float32(KS)), O.fp8_e4m3_encode(v_want / np.float32(VS))
    live = slots >= 0
    _assert_codes_cover_the_format(np.concatenate([k_codes[live].reshape(-1), v_codes[live].reshape(-1)]))
    nblocks, fill = 2 * b, 0xA5
    kc_want = np.full((nblocks, kvh, hd // 16, bs, 16), fill, np.uint8)
    vc_want = np.full((nblocks, kvh, hd, bs), fill, np.uint8)
    for i in np.nonzero(live)[0]:
        blk, off = int(slots[i]) // bs, int(slots[i]) % bs
        kc_want[blk, :, :, off, :] = k_codes[i].reshape(kvh, hd // 16, 16)
        vc_want[blk, :, :, off] = v_codes[i].reshape(kvh, hd)
    kc, vc = be.buf(np.full_like(kc_want, fill)), be.buf(np.full_like(vc_want, fill))
    xb, nb, qb = be.buf(x), be.buf(nw), be.buf(np.zeros((b, nq), dtype=np.float32))
    sb, pb, cb, snb = be.buf(slots), be.buf(pos), be.buf(cos), be.buf(sin)
    if route in ("inline", "neox"):
        fn = be.sym("mrs_dec_qkv_neox_f8" if neox else "mrs_dec_qkv_f8", QKV_F8, CI)
        rc = fn(C.byref(mq), C.byref(mk), C.byref(mv), xb.ptr, k, nb.ptr, 1e-5, qb.ptr, kc.ptr, vc.ptr, sb.ptr, pb.ptr, cb.ptr, snb.ptr, hd, hd // 2, kvh, bs, b, KS, VS, be.stream)
    else:
        img = _act_image(be, Tq, xb, nb, k, b)
        if route == "mm":
            qq, qk, qv = qi_repack(be, Tq, pq, nq, k), qi_repack(be, Tq, pk, nkv, k), qi_repack(be, Tv, pv, nkv, k)
            rc = be.sym("mrs_dec_mm_qkv_f8", MM_QKV_F8, CI)(qq.ptr, Tq, nq, qk.ptr, Tq, nkv, qv.ptr, Tv, nkv, k, img.ptr, qb.ptr, kc.ptr, vc.ptr, sb.ptr, pb.ptr, cb.ptr, snb.ptr,
                                                             hd, hd // 2, kvh, bs, b, KS, VS, be.stream)
        else:
            rc = be.sym("mrs_dec_qkv_img_f8", QKV_IMG_F8, CI)(C.byref(mq), C.byref(mk), C.byref(mv), img.ptr, qb.ptr, kc.ptr, vc.ptr, sb.ptr, pb.ptr, cb.ptr, snb.ptr, hd, hd // 2,
                                                               kvh, bs, b, int(neox), KS, VS, be.stream)
    assert rc == 0, rc
    assert np.array_equal(qb.numpy(), q_want), "q differs from the engine-order oracle"
    gk, gv = kc.numpy().reshape(kc_want.shape), vc.numpy().reshape(vc_want.shape)
    assert np.array_equal(gk, kc_want), (route, "K pages", int((gk != kc_want).sum()))  # (untouched slots keep the fill; slot < 0 wrote nothing)
    assert np.array_equal(gv, vc_want), (route, "V pages", int((gv != vc_want).sum()))


ROUTES = [("inline", 1), ("inline", 2), ("neox", 1), ("img", 2), ("img-neox", 3), ("mm", 3), ("mm", 8)]


@pytest.mark.parametrize("route,b", ROUTES)
def test_page_writes_host_emulation(oracle, route, b):
    check_page_writes(oracle, HostBackend(), "Q4_K", "Q6_K", 4, 2, 512, b, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route,b", [("inline", 1), ("neox", 1), ("img", 2), ("mm", 4)])
def test_page_writes_gpu(oracle, dev, route, b):
    if route == "inline":
        check_page_writes(oracle, GpuBackend(dev), "Q4_K", "Q6_K", 32, 8, 4096, b, route)  # Llama-3-8B's layer shape
    else:
        check_page_writes(oracle, GpuBackend(dev), "Q4_K", "Q6_K", 8, 2, 1024, b, route)


def test_f8_entry_points_refuse_bad_scales_and_old_entries_refuse_the_code_host_emulation(oracle):
    be = HostBackend()
    one = be.buf(np.zeros(64, np.float32))
    for ks, vs in ((0.0, 1.0), (1.0, -1.0), (float("inf"), 1.0), (1.0, float("nan"))):
        assert be.sym("mrs_dec_attention_f8", ATTN_F8, CI)(one.ptr, None, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, 1, 1.0, one.ptr, one.ptr, 32, 32, 1, 1, 128,
                                                            1, 128, 4096, 4096, 0, ks, vs, be.stream) == -1
        assert be.sym("mrs_prefill_attention_exact_f8", PA_F8, CI)(one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, 1, 1, 1, 128, 32, 128, 4096, 4096, 1.0, 32, 0, 0, ks, vs,
                                                                    be.stream) == -1
    assert be.sym("mrs_dec_attention", ATTN2, CI)(one.ptr, None, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, 1, 1.0, one.ptr, one.ptr, 32, 32, 1, 1, 128, 1, 128,
                                                   4096, 4096, 3, 0, be.stream) == -1
    assert be.sym("mrs_prefill_attention_exact", PA, CI)(one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, one.ptr, 1, 1, 1, 128, 32, 128, 4096, 4096, 1.0, 32, 3, 0, 0, be.stream) == -1


# ------------------------------------------------------------------------------------------------ attention
def _pages(rng, nblocks, kvh, bt_rows, ctxs):
    """random non-NaN codes in the slots a context names, the NaN code everywhere else (slots at or past the context, blocks no table entry names), K and V"""
    hd, bs = 128, 32
    codes = lambda shape: rng.integers(0, 0x7F, shape, dtype=np.uint8) | (rng.integers(0, 2, shape, dtype=np.uint8) << 7)  # 0x7F / 0xFF (NaN) never drawn
    kc, vc = np.full((nblocks, kvh, hd // 16, bs, 16), NAN, np.uint8), np.full((nblocks, kvh, hd, bs), NAN, np.uint8)
    for row, ctx in zip(bt_rows, ctxs):
        for pos in range(ctx):
            blk, off = int(row[pos // bs]), pos % bs
            kc[blk, :, :, off, :] = codes((kvh, hd // 16, 16))
            vc[blk, :, :, off] = codes((kvh, hd))
    # keep the scores moderate: K exponents at most 2^0 (codes below 0x40 in magnitude)
    mag = kc & 0x7F
    kc = np.where((kc & 0x7F) != NAN, (kc & 0x80) | (mag % 0x40), kc).astype(np.uint8)
    return kc, vc


def _gather(O, kc, vc, row, ctx):
    pos = np.arange(ctx)
    blk, off = row[pos // 32], pos % 32
    k = (O.fp8_e4m3_decode(kc[blk, :, :, off, :]) * np.float32(KS)).astype(np.float32).reshape(ctx, kc.shape[1], -1)
    v = (O.fp8_e4m3_decode(vc[blk, :, :, off]) * np.float32(VS)).astype(np.float32)
    return k, v


def check_attention(O, be, heads, kvh, ctxs, max_ctx, window=0, n_out=24):
    hd, bs, b = 128, 32, len(ctxs)
    nq = heads * hd
    rng = np.random.default_rng(heads + kvh + sum(ctxs) + window)
    mbs = (max_ctx + bs - 1) // bs
    nblocks = b * mbs + 1
    bt_np = rng.permutation(nblocks - 1)[: b * mbs].reshape(b, mbs).astype(np.uint32) + 1  # permuted; block 0 is never named
    kc_np, vc_np = _pages(rng, nblocks, kvh, bt_np, ctxs)
    kc, vc, bt, cl = be.buf(kc_np), be.buf(vc_np), be.buf(bt_np), be.buf(np.asarray(ctxs, dtype=np.uint32))
    q_np = (rng.standard_normal((b, nq)) * 0.5).astype(np.float32)
    q = be.buf(q_np)
    splits = be.sym("mrs_decode_attention_max_splits", [CI], CI)(max_ctx)
    po, pm, pl = be.buf(np.zeros((b, heads, splits, hd), np.float32)), be.buf(np.zeros((b, heads, splits), np.float32)), be.buf(np.zeros((b, heads, splits), np.float32))
    ticket = be.buf(np.zeros(b * kvh, np.uint32))
    scale = np.float32(1.0 / np.sqrt(np.float32(hd)))
    nimg = be.sym("mrs_dec_act_image_bytes", [CI, CI], C.c_size_t)(nq, b)
    img, got = be.buf(np.zeros(nimg, np.uint8)), be.buf(np.full((b, nq), np.nan, np.float32))
    fn = be.sym("mrs_dec_attention_f8", ATTN_F8, CI)
    even = (heads // kvh) % 2 == 0
    for rep in range(2):  # twice: the ticket must be back at zero
        rc = fn(got.ptr, img.ptr, ticket.ptr, po.ptr, pm.ptr, pl.ptr, q.ptr, kc.ptr, vc.ptr, kvh, scale, bt.ptr, cl.ptr, bs, max_ctx, b, heads, hd, mbs, nq, kvh * hd * bs, hd * bs,
                window, KS, VS, be.stream)
        assert rc == (1 if even else 0)
        assert not ticket.numpy().any()
    res = got.numpy()
    bpw = 1 if mbs <= 64 else (mbs + 63) // 64
    for i, ctx in enumerate(ctxs):
        k, v = _gather(O, kc_np, vc_np, bt_np[i], ctx)
        eng = O.attention_engine(q_np[i].reshape(heads, hd), k, v, scale, bpw, window)
        assert np.isfinite(eng).all()
        assert np.array_equal(res[i].reshape(heads, hd), eng), ("engine-order oracle", i, ctx, float(np.abs(res[i].reshape(heads, hd) - eng).max()))
    if not even:
        return
    t = O.Q4_K
    packed = _weights(O, t, n_out, nq, 7)
    keep, m = repack(be, O, t, packed, n_out, nq)
    base = rng.standard_normal((b, n_out)).astype(np.float32)
    o_ref, o_img = be.buf(base.copy()), be.buf(base.copy())
    assert be.sym("mrs_dec_proj", PROJ, CI)(C.byref(m), n_out, None, got.ptr, nq, None, 0.0, o_ref.ptr, n_out, 1, 0.5, None, b, be.stream) == 0
    assert be.sym("mrs_dec_proj_img", PROJ_IMG, CI)(C.byref(m), n_out, img.ptr, o_img.ptr, n_out, 1, 0.5, b, be.stream) == 0
    np.testing.assert_array_equal(o_img.numpy(), o_ref.numpy())


# G = 1 / 2 / 4 / 8; contexts at the block edges; several blocks per split (max_ctx 4096); a window that starts inside a block (70 - 45 = 25, 200 - 45 = 155)
ATTN_CASES = [(2, 2, [1, 31, 32, 33, 70], 96, 0), (4, 2, [70, 33], 96, 0), (4, 1, [32, 1], 64, 0), (8, 1, [70, 31], 96, 0), (4, 2, [2300], 4096, 0), (4, 2, [70, 200, 40], 224, 45)]


@pytest.mark.parametrize("heads,kvh,ctxs,max_ctx,window", ATTN_CASES)
def test_decode_attention_host_emulation(oracle, heads, kvh, ctxs, max_ctx, window):
    check_attention(oracle, HostBackend(), heads, kvh, ctxs, max_ctx, window)


@pytest.mark.gpu
@pytest.mark.parametrize("heads,kvh,ctxs,max_ctx,window", ATTN_CASES + [(32, 8, [700, 3, 515], 1024, 0)])
def test_decode_attention_gpu(oracle, dev, heads, kvh, ctxs, max_ctx, window):
    check_attention(oracle, GpuBackend(dev), heads, kvh, ctxs, max_ctx, window, n_out=256)


def check_prompt_attention(O, be, heads, kvh, T, max_ctx, window=0, start=0, f8=True, n_rows=6):
    """mrs_prefill_attention_exact_f8 for T prompt tokens at positions start .. start + T - 1 == mrs_dec_attention_f8 at each position (same pages), bit for bit.
    f8 = False: the same body on bf16 pages through the 16-bit entry points (the control of the fallback case)."""
    hd, bs = 128, 32
    nq = heads * hd
    rng = np.random.default_rng(heads + kvh + T + max_ctx + start)
    mbs = (max_ctx + bs - 1) // bs
    used = (start + T + bs - 1) // bs
    nblocks = used + 2
    row = np.zeros(mbs, np.uint32)
    row[:used] = rng.permutation(nblocks - 1)[:used].astype(np.uint32) + 1  # entries past the prompt name block 0 (NaN codes); no kernel may read through them
    if f8:
        kc_np, vc_np = _pages(rng, nblocks, kvh, [row], [start + T])
    else:
        kc_np = O.to_bf16_bits((rng.standard_normal((nblocks, kvh, hd // 8, bs, 8)) * 0.7).astype(np.float32))
        vc_np = O.to_bf16_bits(rng.standard_normal((nblocks, kvh, hd, bs)).astype(np.float32))
    kc, vc, bt = be.buf(kc_np), be.buf(vc_np), be.buf(row.reshape(1, mbs))
    q_np = (rng.standard_normal((T, nq)) * 0.5).astype(np.float32)
    q = be.buf(q_np)
    ctx = np.arange(start + 1, start + T + 1, dtype=np.uint32)
    cl = be.buf(ctx)
    scale = np.float32(1.0 / np.sqrt(np.float32(hd)))
    got = be.buf(np.full((T, nq), np.nan, np.float32))
    mpc = start + T if (heads + T) % 2 else 0
    if f8:
        rc = be.sym("mrs_prefill_attention_exact_f8", PA_F8, CI)(q.ptr, kc.ptr, vc.ptr, bt.ptr, cl.ptr, got.ptr, T, heads, kvh, hd, bs, nq, kvh * hd * bs, hd * bs, scale, max_ctx,
                                                                  window, mpc, KS, VS, be.stream)
    else:
        rc = be.sym("mrs_prefill_attention_exact", PA, CI)(q.ptr, kc.ptr, vc.ptr, bt.ptr, cl.ptr, got.ptr, T, heads, kvh, hd, bs, nq, kvh * hd * bs, hd * bs, scale, max_ctx, 1,
                                                            window, mpc, be.stream)
    assert rc == 0, rc
    res = got.numpy()
    assert np.isfinite(res).all()
    splits = be.sym("mrs_decode_attention_max_splits", [CI], CI)(max_ctx)
    po, pm, pl = be.buf(np.zeros((1, heads, splits, hd), np.float32)), be.buf(np.zeros((1, heads, splits), np.float32)), be.buf(np.zeros((1, heads, splits), np.float32))
    ticket = be.buf(np.zeros(kvh, np.uint32))
    rows = sorted(set([0, 1, T // 3, T // 2, T - 2, T - 1][:n_rows]) & set(range(T)))
    for t in rows:
        one, c1, q1 = be.buf(np.full((1, nq), np.nan, np.float32)), be.buf(ctx[t:t + 1].copy()), be.buf(q_np[t:t + 1].copy())
        if f8:
            rc = be.sym("mrs_dec_attention_f8", ATTN_F8, CI)(one.ptr, None, ticket.ptr, po.ptr, pm.ptr, pl.ptr, q1.ptr, kc.ptr, vc.ptr, kvh, scale, bt.ptr, c1.ptr, bs, max_ctx, 1, heads,
                                                              hd, mbs, nq, kvh * hd * bs, hd * bs, window, KS, VS, be.stream)
        else:
            rc = be.sym("mrs_dec_attention", ATTN2, CI)(one.ptr, None, ticket.ptr, po.ptr, pm.ptr, pl.ptr, q1.ptr, kc.ptr, vc.ptr, kvh, scale, bt.ptr, c1.ptr, bs, max_ctx, 1, heads, hd,
                                                         mbs, nq, kvh * hd * bs, hd * bs, 1, window, be.stream)
        assert rc == 0
        assert np.array_equal(res[t], one.numpy()[0]), (t, float(np.abs(res[t] - one.numpy()[0]).max()))


PROMPT_CASES = [(4, 1, 33, 96, 0, 0), (4, 2, 40, 96, 0, 20), (2, 2, 70, 96, 0, 0), (8, 1, 33, 64, 0, 20), (2, 1, 70, 128, 0, 20), (4, 1, 70, 128, 27, 0), (8, 2, 40, 4096, 0, 0)]


@pytest.mark.parametrize("heads,kvh,T,max_ctx,window,start", PROMPT_CASES)
def test_prompt_attention_equals_decode_attention_host_emulation(oracle, heads, kvh, T, max_ctx, window, start):
    check_prompt_attention(oracle, HostBackend(), heads, kvh, T, max_ctx, window, start)


@pytest.mark.gpu
@pytest.mark.parametrize("heads,kvh,T,max_ctx,window,start", PROMPT_CASES + [(32, 8, 300, 1024, 0, 100)])
def test_prompt_attention_equals_decode_attention_gpu(oracle, dev, heads, kvh, T, max_ctx, window, start):
    check_prompt_attention(oracle, GpuBackend(dev), heads, kvh, T, max_ctx, window, start)


@pytest.mark.gpu
@pytest.mark.parametrize("f8", [True, False], ids=["f8", "bf16-control"])
def test_prompt_attention_vector_alu_fallback_gpu(oracle, dev, f8):
    """start + T > 32768 under max_context_len 40960: the per-block maxima of the matrix-core kernel no longer fit LDS and the launcher takes prefill_attn_exact_kernel
    (several blocks per split).  The bf16 twin is the control: the same shape through the 16-bit entry points."""
    check_prompt_attention(oracle, GpuBackend(dev), 2, 1, 40, 40960, 0, 32768 - 20, f8=f8, n_rows=3)


# ------------------------------------------------------------------------------------------------ the codec on the device
@pytest.mark.gpu
def test_all_256_codes_through_a_page_gpu(oracle, dev):
    """Every code as a V element read back through attention with a one-hot probability (context 1: p = 1, out = 1 * v / 1): f32(decode(code) * v_scale) for the 254
    non-NaN codes -- the bar a hardware convert has to clear to stand in for the integer decode of csrc/common.cuh.  K carries the same codes (finite scores only)."""
    O, be = oracle, GpuBackend(dev)
    hd, bs, kvh, heads, b = 128, 32, 1, 1, 2
    codes = np.arange(256, dtype=np.uint8)
    live = (codes & 0x7F) != NAN
    vc_np = np.full((b + 1, kvh, hd, bs), NAN, np.uint8)
    kc_np = np.full((b + 1, kvh, hd // 16, bs, 16), NAN, np.uint8)
    for i in range(b):  # sequence i: token 0 of block i + 1 holds codes 128 i .. 128 i + 127 over the head's dims
        vc_np[i + 1, 0, :, 0] = codes[128 * i: 128 * (i + 1)]
        kc_np[i + 1, 0, :, 0, :] = np.where(live, codes, 0)[128 * i: 128 * (i + 1)].reshape(hd // 16, 16)
    bt_np = np.arange(1, b + 1, dtype=np.uint32).reshape(b, 1)
    kc, vc, bt, cl = be.buf(kc_np), be.buf(vc_np), be.buf(bt_np), be.buf(np.ones(b, np.uint32))
    q = be.buf(np.full((b, hd), 0.01, np.float32))
    splits = be.sym("mrs_decode_attention_max_splits", [CI], CI)(32)
    po, pm, pl = be.buf(np.zeros((b, 1, splits, hd), np.float32)), be.buf(np.zeros((b, 1, splits), np.float32)), be.buf(np.zeros((b, 1, splits), np.float32))
    ticket, got = be.buf(np.zeros(b, np.uint32)), be.buf(np.full((b, hd), np.nan, np.float32))
    rc = be.sym("mrs_dec_attention_f8", ATTN_F8, CI)(got.ptr, None, ticket.ptr, po.ptr, pm.ptr, pl.ptr, q.ptr, kc.ptr, vc.ptr, kvh, 1.0, bt.ptr, cl.ptr, bs, 32, b, heads, hd, 1, hd,
                                                      kvh * hd * bs, hd * bs, 0, KS, VS, be.stream)
    assert rc == 0
    res = got.numpy().reshape(-1)
    want = (O.fp8_e4m3_decode(codes) * np.float32(VS)).astype(np.float32)
    # value equality: code 0x80 (-0) comes back as +0 through the chain's 0 + 1 * (-0); every other live code is non-zero, so equal values are equal bits
    assert np.array_equal(res[live], want[live]), [(int(c), float(res[c]), float(want[c])) for c in np.nonzero(live & (res != want))[0]]
    assert np.isnan(res[~live]).all()
    # the matrix-core prompt kernel decodes with its own convert (one byte at a time): the same codes as one-token prompts (T = 1, context 1) through
    # mrs_prefill_attention_exact_f8, K and V
    for i in range(b):
        out1 = be.buf(np.full((1, hd), np.nan, np.float32))
        row, c1 = be.buf(bt_np[i:i + 1].copy()), be.buf(np.ones(1, np.uint32))
        assert be.sym("mrs_prefill_attention_exact_f8", PA_F8, CI)(q.ptr, kc.ptr, vc.ptr, row.ptr, c1.ptr, out1.ptr, 1, heads, kvh, hd, bs, hd, kvh * hd * bs, hd * bs, 1.0, 32, 0, 1,
                                                                    KS, VS, be.stream) == 0
        r1, sl = out1.numpy().reshape(-1), slice(128 * i, 128 * (i + 1))
        assert np.array_equal(r1[live[sl]], want[sl][live[sl]]), ("prompt kernel", i)
        assert np.isnan(r1[~live[sl]]).all()
