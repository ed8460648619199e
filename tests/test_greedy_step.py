"""The greedy step of the batch-1 decode graph, launch by launch: arg-max, state advance, embedding row.

  mrs_sample_greedy_advance  (csrc/ext_decode.hip: argmax_partial_kernel + sample_advance_kernel)   arg-max over [b][vocab] logits, then the device-resident state update
  mrs_dec_proj_argmax        (csrc/ext_dec.hip, dec_gemv_kernel<1, EPI_STORE>)                      lm_head with the arg-max folded into its epilogue as a packed key
  mrs_sample_advance_embed   (sample_advance_embed_kernel)                                          consumes the key, advances the state, gathers the next embedding row
  mrs_embedding              (embedding_kernel)                                                     rows of an f32 / f16 / bf16 / Q4_K / Q5_K / Q6_K / Q8_0 table -> f32

No tolerances: ids, state words and embedding rows are compared for EQUALITY (floats through their uint32 view).

  * arg-max: a plain loop with the rule of the reference's argmax_f32 (mistralrs-core/src/sampler.rs:513-529): strict `>`, so the largest value at the LOWEST index, and
    -0.0 == +0.0.  Defined over finite values and -inf; a NaN, a +inf or a row without a finite entry is an error in the reference and out of scope here (ref_argmax
    refuses such a row instead of inventing an answer).
  * state: a restatement of the slot arithmetic of inputs_processor.rs:900-922 (slot = table[pos / bs] * bs + pos % bs), positions + 1, context_lens = pos + 1; past the
    block table the kernels write the pad slot -1 where the reference panics (a graph replayed past its buffers must not write into another sequence's page).
  * embedding rows: oracle.dequantize (tied to the formats by tests/test_oracle.py), numpy's f16 -> f32 and the oracle's bf16 -> f32.
  * lm_head values: mrs_dec_proj (mode 0) on the same inputs and oracle.gemv_engine(oracle.rms_norm_engine(x)), both bit for bit.

Every body runs on the wave64 host emulation (CPU suite) and on the MI355X (`-m gpu`).  Every output array carries one guard element behind its last live one.

Start positions of the state tests are the positions BEFORE the call: 30 -> 31 stays in its block, 31 -> 32 is the first slot of the next block, 94 -> 95 is the last slot
of the table, 95 -> 96 and 96 -> 97 have no block left.

lm_head and -0.0: pack_max_key ranks -0.0 with +0.0, but the GEMV cannot produce a -0.0 logit to show it.  A Q8_0 row of all-zero quants with a negative d gives integer
block sums of 0, and every f32 partial is added to an accumulator that starts at +0.0: (+0.0) + (-0.0) = +0.0.  Measured on the host emulation (see
test_lm_head_zero_quant_rows_host_emulation): the stored logit is +0.0 for d < 0 as for d > 0, the two rows tie as equal values, and the lower index wins either way."""
import ctypes as C

import numpy as np
import pytest

from tests.abi_backends import GpuBackend, HostBackend
from tests.test_dec_engine import PROJ, Mat, repack

VP, I, F = C.c_void_p, C.c_int, C.c_float
GREEDY = [VP, I, I, VP, VP, I, VP, VP, VP, VP, VP, I, I, VP, VP]
ADV_EMBED = [VP, VP, I, VP, VP, VP, VP, VP, I, I, VP, VP, I, VP, I, VP]
PROJ_ARGMAX = [C.POINTER(Mat), I, VP, I, VP, F, VP, I, VP, VP]
EMBED = [VP, I, VP, VP, I, I, VP]
SENT = -77777777          # guard elements of the integer arrays
FSENT = np.float32(-12345.0)  # and of the float ones
T_F32, T_F16, T_Q4_0, T_BF16 = 0, 1, 2, 30


# ------------------------------------------------------------------------------------------------ references
def ref_argmax(row):
    """argmax_f32 (sampler.rs:513-529): strict `>` from -inf on, first maximum wins; -0.0 > +0.0 and +0.0 > -0.0 are both false"""
    best, best_v = None, float("-inf")
    for i, v in enumerate(np.asarray(row, dtype=np.float32).tolist()):
        assert v == v and v != float("inf"), "NaN / +inf logits are an error in the reference: out of scope"
        if v > best_v:
            best, best_v = i, v
    assert best is not None, "a row without a finite logit is an error in the reference: out of scope"
    return best


def _same(got, want, what):
    got = np.ascontiguousarray(got)
    if got.dtype != want.dtype:
        assert got.dtype.itemsize == want.dtype.itemsize, (what, got.dtype, want.dtype)
        got = got.view(want.dtype)  # torch has no uint32: the same words
    assert np.array_equal(got.reshape(-1), want.reshape(-1)), (what, got.reshape(-1)[:80], want.reshape(-1)[:80])


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError((what, f"{len(bad)} of {g.size} words differ; first at {i}: got {got[i]!r} (0x{int(g[i]):08x}), want {want[i]!r} (0x{int(w[i]):08x})"))


class DecodeState:
    """The device-resident decode state of b sequences and its reference: block_size 32, 3 blocks per sequence, non-monotonic block ids, distinct per sequence."""
    BS, MB = 32, 3

    def __init__(self, be, b, starts, step=0, stride=4, tokens=True):
        self.b, self.stride, self.tokens = b, stride, tokens
        self.table = np.array([[7 + 10 * c, 2 + 10 * c, 5 + 10 * c] for c in range(b)], dtype=np.uint32)
        pos = np.array([starts[c % len(starts)] for c in range(b)], dtype=np.int32)
        self.h = {"next_ids": np.full(b + 1, SENT, np.int32),
                  "tokens_out": np.full(b * stride + 1, SENT, np.int32),  # the word after every row is the next row's first, or the guard
                  "step_counter": np.array([step, SENT], np.int32),
                  "positions": np.append(pos, np.int32(SENT)).astype(np.int32),
                  "context_lens": np.append(pos + 1, 0xDEADBEEF).astype(np.uint32),
                  "slot_mapping": np.full(b + 1, SENT, np.int64),
                  "scratch": np.append(np.zeros(b, np.int64), np.int64(SENT))}
        self.d = {k: be.buf(v) for k, v in self.h.items()}
        self.tab = be.buf(self.table)

    def ptr(self, k):
        if k == "tokens_out" and not self.tokens:
            return None
        return self.d[k].ptr

    def args(self):
        """(next_ids, tokens_out, tokens_out_stride, step_counter, positions, context_lens, slot_mapping, block_tables, max_blocks, block_size, scratch)"""
        return (self.ptr("next_ids"), self.ptr("tokens_out"), self.stride, self.ptr("step_counter"), self.ptr("positions"), self.ptr("context_lens"),
                self.ptr("slot_mapping"), self.tab.ptr, self.MB, self.BS, self.ptr("scratch"))

    def advance(self, ids):
        """what one greedy step does to the state, given the ids it chose"""
        h, step = self.h, int(self.h["step_counter"][0])
        for c, tok in enumerate(ids):
            h["next_ids"][c] = tok
            if self.tokens and step < self.stride:
                h["tokens_out"][c * self.stride + step] = tok
            pos = int(h["positions"][c]) + 1
            h["positions"][c] = pos
            h["context_lens"][c] = pos + 1
            blk = pos // self.BS
            h["slot_mapping"][c] = int(self.table[c][blk]) * self.BS + pos % self.BS if blk < self.MB else -1
        h["step_counter"][0] = step + 1  # by one per call, whatever b is

    def check(self):
        for k, want in self.h.items():  # (scratch: all zero again, its guard untouched)
            _same(self.d[k].numpy(), want, k)
        _same(self.tab.numpy(), self.table, "block_tables")


def upload_at(be, a, mis=0):
    """`a` on the backend with its first element `mis` floats past a 16-byte boundary -> (buffer, address)"""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = be.buf(np.zeros(flat.size + 8, flat.dtype))
    off = (-(buf.ptr // 4) + mis) % 4
    host = np.zeros(flat.size + 8, flat.dtype)
    host[off:off + flat.size] = flat
    buf.write(host)
    assert (buf.ptr + 4 * off) % 16 == 4 * mis
    return buf, buf.ptr + 4 * off


def greedy(be, st, logits, mis=0):
    """one mrs_sample_greedy_advance on `logits` [b][vocab]; checks ids and the whole state against the references; returns the ids"""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    b, vocab = logits.shape
    keep, ptr = upload_at(be, logits, mis)
    assert be.sym("mrs_sample_greedy_advance", GREEDY, C.c_int)(ptr, vocab, b, *st.args(), be.stream) == 0
    want = [ref_argmax(r) for r in logits]
    st.advance(want)
    st.check()
    return want


# ------------------------------------------------------------------------------------------------ 1. mrs_sample_greedy_advance: arg-max
def _geom(vocab):
    """the launch geometry of mrs_sample_greedy_advance: workgroups per row (<= 256), float4s per row, float4s per workgroup"""
    gx = min(max((vocab + 2047) // 2048, 1), 256)
    n4 = vocab // 4
    return gx, n4, (n4 + gx - 1) // gx


def _background(rng, b, vocab):
    return (-np.abs(rng.standard_normal((b, vocab))) - 1.0).astype(np.float32)


def _plants(vocab):
    gx, n4, per = _geom(vocab)
    return sorted({i for i in (0, vocab - 1, 4 * n4 - 1, 4 * per) if 0 <= i < vocab})  # first, last (in the tail), last of the float4 body, a workgroup boundary


def check_planted(be, vocab, b):
    """the winner at index 0, at vocab - 1, at the end of the float4 body and at a workgroup boundary, on a background of -|normal| - 1: as the only non-negative entry (2.5)
    and as the largest of an all-negative row (-0.5).  Every call reuses the same state and scratch: a later call must give the new answer."""
    rng = np.random.default_rng(1000 * vocab + b)
    st = DecodeState(be, b, [3, 40, 77], step=0, stride=5)
    plants = _plants(vocab)
    for shift in range(len(plants)):
        for val, mis in ((2.5, 0), (-0.5, 1 + shift % 3)):
            idx = [plants[(c + shift) % len(plants)] for c in range(b)]
            lg = _background(rng, b, vocab)
            lg[np.arange(b), idx] = val
            assert greedy(be, st, lg, mis) == idx


VOCABS = [5, 7, 2048, 2049, 2051, 4099]  # only the tail loop (5, 7); one workgroup exactly; tails of 1 and 3; odd: rows 1.. are not 16-byte aligned
BATCHES = [1, 3, 8, 64]
BIG_VOCAB = 524288 + 3                    # the cap of 256 workgroups per row


@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("vocab", VOCABS)
def test_argmax_planted_host_emulation(vocab, b):
    check_planted(HostBackend(), vocab, b)


def test_argmax_planted_big_vocab_host_emulation():
    check_planted(HostBackend(), BIG_VOCAB, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("vocab", VOCABS)
def test_argmax_planted_gpu(dev, vocab, b):
    check_planted(GpuBackend(dev), vocab, b)


@pytest.mark.gpu
def test_argmax_planted_big_vocab_gpu(dev):
    check_planted(GpuBackend(dev), BIG_VOCAB, 1)


def _tie_pairs(vocab):
    """index pairs (lo, hi) that hold the same maximum: in different workgroups, on both sides of a workgroup boundary, in the first and the last thread's float4, inside
    one float4, in the body and in the tail, both in the tail"""
    gx, n4, per = _geom(vocab)
    pairs = []
    if gx > 1:
        pairs += [(min(5, 4 * per - 1), 4 * per * (gx - 1) + 2), (4 * per - 1, 4 * per)]
    if n4 >= 3:
        pairs.append((0, 4 * (n4 - 1) + 3))
    q = n4 // 2
    if n4 >= 1:
        pairs.append((4 * q + 1, 4 * q + 3))
    if vocab % 4:
        pairs.append((min(4 * q + 2, 4 * n4 - 1), vocab - 1))
    if vocab % 4 >= 2:
        pairs.append((4 * n4, vocab - 1))
    assert all(0 <= lo < hi < vocab for lo, hi in pairs), pairs
    return pairs


def _special_rows(vocab, seed, lean=False):
    """rows and the index the rule gives (also recomputed by ref_argmax: the two must agree).  lean (the 2 MB rows of the largest vocabulary): what depends on the number
    of workgroups -- the first and the last one, a boundary, the tail behind the last one"""
    rng = np.random.default_rng(seed)
    rows, want = [], []
    for i in ((vocab - 1,) if lean else sorted({0, vocab // 2, vocab - 1})):  # -inf everywhere but one finite entry
        r = np.full(vocab, -np.inf, np.float32)
        r[i] = -1e30
        rows.append(r); want.append(i)
    for v in ((-2.0,) if lean else (-2.0, 1.5, 0.0, -0.0)):  # every entry equal: index 0
        rows.append(np.full(vocab, v, np.float32)); want.append(0)
    pairs = _tie_pairs(vocab)
    for n, (lo, hi) in enumerate(pairs[:2] + pairs[-2:-1] if lean else pairs):
        kinds = ((1.25, 1.25), (-0.5, -0.5), (-0.0, 0.0), (0.0, -0.0))  # the zero cases: everything else negative, the zeros are equal, the lower index wins
        for vlo, vhi in (kinds[n::2] if lean else kinds):
            r = _background(rng, 1, vocab)[0]
            r[lo], r[hi] = vlo, vhi
            rows.append(r); want.append(lo)
    return np.stack(rows), want


def check_special(be, vocab, batched=True):
    rows, want = _special_rows(vocab, vocab, lean=not batched)
    assert len(rows) <= 64
    if batched:  # all rows in one launch (an odd vocab: the rows after the first take the scalar path)
        st = DecodeState(be, len(rows), [3, 40, 77], step=0, stride=2)
        assert greedy(be, st, rows) == want
    st = DecodeState(be, 1, [9], step=0, stride=2)
    for i, r in enumerate(rows):  # one row per launch, 16-byte aligned and not
        for mis in ((0, 1 + i % 3) if batched else (0,)):
            assert greedy(be, st, r[None], mis) == [want[i]], (i, mis)


@pytest.mark.parametrize("vocab", VOCABS)
def test_argmax_ties_zeros_minus_inf_host_emulation(vocab):
    check_special(HostBackend(), vocab)


def test_argmax_ties_zeros_minus_inf_big_vocab_host_emulation():
    check_special(HostBackend(), BIG_VOCAB, batched=False)


@pytest.mark.gpu
@pytest.mark.parametrize("vocab", VOCABS)
def test_argmax_ties_zeros_minus_inf_gpu(dev, vocab):
    check_special(GpuBackend(dev), vocab)


@pytest.mark.gpu
def test_argmax_ties_zeros_minus_inf_big_vocab_gpu(dev):
    check_special(GpuBackend(dev), BIG_VOCAB, batched=False)


def check_greedy_refusals(be):
    """b = 0 and b = 65 are refused (-1) and nothing is touched"""
    st = DecodeState(be, 64, [3], step=1)
    lg = be.buf(np.zeros((65, 7), np.float32))
    fn = be.sym("mrs_sample_greedy_advance", GREEDY, C.c_int)
    for b in (0, 65, -1):
        assert fn(lg.ptr, 7, b, *st.args(), be.stream) == -1
    st.check()


def test_greedy_refusals_host_emulation():
    check_greedy_refusals(HostBackend())


@pytest.mark.gpu
def test_greedy_refusals_gpu(dev):
    check_greedy_refusals(GpuBackend(dev))


# ------------------------------------------------------------------------------------------------ 2. state advance
STARTS = [30, 31, 94, 95, 96]


def check_state_greedy(be, b):
    """mrs_sample_greedy_advance: every start position in every sequence slot; tokens_out_stride 4 at step_counter 3 (written) and 4 (dropped), tokens_out == NULL; two calls"""
    rng = np.random.default_rng(b)
    for rot in range(len(STARTS)):
        starts = STARTS[rot:] + STARTS[:rot]
        for step, tokens in ((3, True), (4, True), (2, False)):
            st = DecodeState(be, b, starts, step=step, stride=4, tokens=tokens)
            for call in range(2):
                lg = _background(rng, b, 7)
                idx = [int(i) for i in rng.integers(0, 7, b)]
                lg[np.arange(b), idx] = 1.0
                assert greedy(be, st, lg) == idx
            assert int(st.d["step_counter"].numpy()[0]) == step + 2


@pytest.mark.parametrize("b", [1, 3])
def test_state_advance_greedy_host_emulation(b):
    check_state_greedy(HostBackend(), b)


@pytest.mark.gpu
@pytest.mark.parametrize("b", [1, 3])
def test_state_advance_greedy_gpu(dev, b):
    check_state_greedy(GpuBackend(dev), b)


def make_table(O, t, vocab, K, seed):
    """an embedding table of type t -> (the array to upload, its f32 rows [vocab][K]).  Quantized: random_blocks (negative d, non-trivial dmin); 16-bit and f32: random
    finite bit patterns plus subnormals, +-0 and the largest finite values."""
    rng = np.random.default_rng(seed)
    if t == T_F32:
        bits = rng.integers(0, 1 << 32, (vocab, K), dtype=np.uint64).astype(np.uint32)
        bits[(bits & 0x7f800000) == 0x7f800000] &= 0xbfffffff  # no inf / NaN
        bits.reshape(-1)[:8] = [0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x7f7fffff, 0xff7fffff, 0x00800000]
        f = bits.view(np.float32)
        return f, f.copy()
    if t in (T_F16, T_BF16):
        emask, fix = (0x7c00, 0xbfff) if t == T_F16 else (0x7f80, 0xbfff)
        bits = rng.integers(0, 1 << 16, (vocab, K), dtype=np.uint32).astype(np.uint16)
        bits[(bits & emask) == emask] &= fix
        special = [0, 0x8000, 1, 0x8001, 0x03ff, 0x83ff, 0x7bff, 0xfbff] if t == T_F16 else [0, 0x8000, 1, 0x8001, 0x007f, 0x807f, 0x7f7f, 0xff7f]
        for r in (0, vocab - 1):
            bits[r, :8] = special            # subnormals, +-0, the largest finite value of either sign
            bits[r, K - 8:] = special[::-1]
        f = bits.view(np.float16).astype(np.float32) if t == T_F16 else O.from_bf16_bits(bits)
        assert np.isfinite(f).all()
        return bits, np.ascontiguousarray(f, dtype=np.float32)
    blocks = O.random_blocks(t, vocab, K, seed=seed)
    return blocks, O.dequantize(t, blocks, K).reshape(vocab, K)


def _embed_types(O):
    return [T_F32, T_F16, T_BF16, O.Q4_K, O.Q5_K, O.Q6_K, O.Q8_0]


def check_state_embed(O, be, ti, K):
    """mrs_sample_advance_embed alone, the key written by hand ((anything) << 32 | 0x7fffffff - id): id, state at every start position, tokens_out written / dropped / NULL,
    key consumed, h_next == the row of that id"""
    t = _embed_types(O)[ti]
    vocab = 11
    table, rows = make_table(O, t, vocab, K, seed=100 + ti)
    tb = be.buf(table)
    fn = be.sym("mrs_sample_advance_embed", ADV_EMBED, C.c_int)
    ids = [10, 0, 7, 0, 10, 3]
    n = 0
    for start in STARTS:
        for step, tokens in ((3, True), (4, True), (2, False)):
            tok = ids[n % len(ids)]
            n += 1
            st = DecodeState(be, 1, [start], step=step, stride=4, tokens=tokens)
            key = np.array([(0x12345678 << 32) | (0x7fffffff - tok), SENT], dtype=np.int64)
            st.d["scratch"].write(key)
            h = be.buf(np.full((2, K), FSENT, np.float32))
            assert fn(*st.args(), tb.ptr, t, h.ptr, K, be.stream) == 0
            st.advance([tok])
            st.check()
            _bits_equal(h.numpy(), np.stack([rows[tok], np.full(K, FSENT, np.float32)]), ("h_next", t, K, tok))


@pytest.mark.parametrize("K", [256, 8448])
@pytest.mark.parametrize("ti", range(7))
def test_state_advance_embed_host_emulation(oracle, ti, K):
    check_state_embed(oracle, HostBackend(), ti, K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 8448])
@pytest.mark.parametrize("ti", range(7))
def test_state_advance_embed_gpu(oracle, dev, ti, K):
    check_state_embed(oracle, GpuBackend(dev), ti, K)


# ------------------------------------------------------------------------------------------------ 3. mrs_dec_proj_argmax
def _activations(rng, k, how):
    x = rng.standard_normal(k).astype(np.float32)
    if how == "negative":
        x = (np.abs(x) + 0.1).astype(np.float32)  # all positive against all-negative weights
    return x, np.abs(1.0 + 0.1 * rng.standard_normal(k)).astype(np.float32)


def _strong_row(rng, x, amp):
    """a weight row whose logit is far above every random row's"""
    return (amp * np.sign(x) * (0.5 + np.abs(rng.standard_normal(x.size)))).astype(np.float32)


def _lm_head(O, t, n, k, how, x, rng):
    """-> (packed rows [n][row bytes], the rows that must share the maximum, lowest first, or None)"""
    small = n <= 4096
    if how == "negative":  # a dense all-negative matrix: every logit is negative, a padded row that contributed 0 would win
        rows = n if small else 501
        assert n % rows == 0
        w = (-np.abs(rng.standard_normal((rows, k))) * 0.05 - 0.01).astype(np.float32)
        return np.tile(O.quantize(t, w).reshape(rows, -1), (n // rows, 1)), None
    if small:
        packed = O.quantize(t, (rng.standard_normal((n, k)) * 0.05).astype(np.float32)).reshape(n, -1)
        amp = 0.2
    else:
        packed = O.random_blocks(t, n, k, seed=n, d_scale=1e-3)
        amp = 1.0
    if how == "random":
        return packed, None
    strong = O.quantize(t, _strong_row(rng, x, amp)[None]).reshape(-1)
    if how == "last":  # the maximum in the last row
        packed[n - 1] = strong
        return packed, [n - 1]
    # the same packed bytes in two rows.  A unit is 4 rows and a launch has at most 256 workgroups of consecutive units: rows 4 * ceil(units / 256) or more apart are in
    # different workgroups (first and last, or two in the middle); tie_near: two rows of one unit (one wave)
    far = 4 * (((n + 3) // 4 + 255) // 256)
    lo, hi = {"tie_far": (1, n - 2), "tie_far_swapped": (n // 2 - 1, n // 2 - 1 + 2 * far), "tie_near": (4 * (n // 4) - 3, 4 * (n // 4) - 2)}[how]
    assert 0 <= lo < hi < n and (hi - lo >= far if how != "tie_near" else lo // 4 == hi // 4)
    if how == "tie_far_swapped":  # which of the two is the copy makes no difference to the bytes; the pair sits elsewhere and the higher row is written first
        packed[hi] = strong
        packed[lo] = packed[hi]
    else:
        packed[lo] = strong
        packed[hi] = packed[lo]
    return packed, [lo, hi]


HOWS = ["random", "negative", "tie_far", "tie_far_swapped", "tie_near", "last"]
LM_SHAPES = [("Q4_K", 33, 512, True), ("Q4_K", 1000, 1024, False), ("Q5_K", 70, 768, True), ("Q6_K", 515, 512, True), ("Q8_0", 257, 512, False)]


def _decode_key(amax_words):
    return 0x7fffffff - (int(amax_words[0]) & 0xffffffff)


def check_proj_argmax(O, be, tname, n, k, norm, how):
    t = getattr(O, tname)
    rng = np.random.default_rng(n + k + HOWS.index(how))
    x, nw = _activations(rng, k, how)
    packed, top = _lm_head(O, t, n, k, how, x, rng)
    keep, m = repack(be, O, t, packed, n, k)
    xb, nb = be.buf(x), (be.buf(nw) if norm else None)
    nptr = nb.ptr if norm else None
    o_plain, o_amax = be.buf(np.full(n + 1, FSENT, np.float32)), be.buf(np.full(n + 1, FSENT, np.float32))
    amax = be.buf(np.array([0, SENT], np.int64))
    assert be.sym("mrs_dec_proj", PROJ, C.c_int)(C.byref(m), n, None, xb.ptr, k, nptr, 1e-5, o_plain.ptr, n, 0, 1.0, None, 1, be.stream) == 0
    assert be.sym("mrs_dec_proj_argmax", PROJ_ARGMAX, C.c_int)(C.byref(m), n, xb.ptr, k, nptr, 1e-5, o_amax.ptr, n, amax.ptr, be.stream) == 0
    got, plain = o_amax.numpy(), o_plain.numpy()
    _bits_equal(got, plain, (tname, n, k, how, "mrs_dec_proj mode 0"))
    assert got[n] == FSENT
    xe = O.rms_norm_engine(x[None], nw, 1e-5)[0] if norm else x
    _bits_equal(got[:n], O.gemv_engine(t, packed, n, k, xe)[0], (tname, n, k, how, "engine-order oracle"))
    words = amax.numpy()
    assert int(words[1]) == SENT
    idx = _decode_key(words)
    assert 0 <= idx < n, (idx, n)
    assert idx == ref_argmax(got[:n]), (tname, n, k, how, idx, ref_argmax(got[:n]))
    # the constructions did what they are for
    if how == "negative":
        assert (got[:n] < 0).all()
    if top:
        assert idx == top[0]
        assert len({int(v) for v in got[top].view(np.uint32)}) == 1 and float(got[top[0]]) > float(np.delete(got[:n], top).max())


# the emulation runs a 250-workgroup launch in seconds: the two larger shapes take the constructions that need their size there (many workgroups; a ragged last unit behind
# 128 full ones), the three small ones take all of them; the MI355X runs every pair
LM_HOST = [(*s, h) for s in LM_SHAPES for h in HOWS if s[1] < 500 or (s[1], h) in ((1000, "tie_far"), (515, "negative"), (515, "tie_far_swapped"))]


@pytest.mark.parametrize("tname,n,k,norm,how", LM_HOST)
def test_proj_argmax_host_emulation(oracle, tname, n, k, norm, how):
    check_proj_argmax(oracle, HostBackend(), tname, n, k, norm, how)


@pytest.mark.gpu
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("tname,n,k,norm", LM_SHAPES + [("Q6_K", 32064, 4096, False)])
def test_proj_argmax_gpu(oracle, dev, tname, n, k, norm, how):
    check_proj_argmax(oracle, GpuBackend(dev), tname, n, k, norm, how)


def check_proj_argmax_refusals(O, be):
    n, k = 16, 512
    t = O.Q4_K
    keep, m = repack(be, O, t, O.random_blocks(t, n, k, seed=1), n, k)
    x, out, amax = be.buf(np.ones(k, np.float32)), be.buf(np.full(n + 1, FSENT, np.float32)), be.buf(np.array([0, SENT], np.int64))
    fn = be.sym("mrs_dec_proj_argmax", PROJ_ARGMAX, C.c_int)
    assert fn(C.byref(m), n, x.ptr, k, None, 0.0, out.ptr, n, None, be.stream) == -1      # amax == NULL
    for bad_n in (n - 1, n // 2, n + 4, 0):
        assert fn(C.byref(m), bad_n, x.ptr, k, None, 0.0, out.ptr, n, amax.ptr, be.stream) == -1  # w->n != n
    assert fn(None, n, x.ptr, k, None, 0.0, out.ptr, n, amax.ptr, be.stream) == -1
    assert (out.numpy() == FSENT).all() and list(amax.numpy()) == [0, SENT]
    assert fn(C.byref(m), n, x.ptr, k, None, 0.0, out.ptr, n, amax.ptr, be.stream) == 0


def test_proj_argmax_refusals_host_emulation(oracle):
    check_proj_argmax_refusals(oracle, HostBackend())


@pytest.mark.gpu
def test_proj_argmax_refusals_gpu(oracle, dev):
    check_proj_argmax_refusals(oracle, GpuBackend(dev))


def check_lm_head_zero_quant_rows(O, be):
    """Can lm_head produce -0.0?  Q8_0 rows of all-zero quants with d = -1 (row 2) and d = +1 (row 9) on all-negative other rows.  The finding (module docstring): both
    logits are +0.0; they are the maximum, equal, and the lower index wins -- in either order of the two rows."""
    t, n, k = O.Q8_0, 13, 512
    rng = np.random.default_rng(7)
    x, _ = _activations(rng, k, "negative")
    for neg_row, pos_row in ((2, 9), (9, 2)):
        packed = O.quantize(t, (-np.abs(rng.standard_normal((n, k))) * 0.05 - 0.01).astype(np.float32)).reshape(n, k // 32, 34).copy()
        packed[neg_row] = 0
        packed[pos_row] = 0
        packed[neg_row, :, 0:2] = np.frombuffer(np.float16(-1.0).tobytes(), np.uint8)
        packed[pos_row, :, 0:2] = np.frombuffer(np.float16(1.0).tobytes(), np.uint8)
        packed = packed.reshape(n, -1)
        keep, m = repack(be, O, t, packed, n, k)
        xb, out, amax = be.buf(x), be.buf(np.full(n + 1, FSENT, np.float32)), be.buf(np.array([0, SENT], np.int64))
        assert be.sym("mrs_dec_proj_argmax", PROJ_ARGMAX, C.c_int)(C.byref(m), n, xb.ptr, k, None, 0.0, out.ptr, n, amax.ptr, be.stream) == 0
        got = out.numpy()[:n]
        _bits_equal(got, O.gemv_engine(t, packed, n, k, x)[0], "engine-order oracle")
        assert [int(v) for v in got[[neg_row, pos_row]].view(np.uint32)] == [0, 0], "a zero-quant row with d < 0 stores +0.0, like d > 0"
        assert (np.delete(got, [neg_row, pos_row]) < 0).all()
        assert _decode_key(amax.numpy()) == ref_argmax(got) == 2


def test_lm_head_zero_quant_rows_host_emulation(oracle):
    check_lm_head_zero_quant_rows(oracle, HostBackend())


@pytest.mark.gpu
def test_lm_head_zero_quant_rows_gpu(oracle, dev):
    check_lm_head_zero_quant_rows(oracle, GpuBackend(dev))


# ------------------------------------------------------------------------------------------------ 4. mrs_dec_proj_argmax -> mrs_sample_advance_embed
def check_chain(O, be, ti, K, tname, n, k, norm, starts):
    """one launch of each on a zeroed amax, twice in a row on the same amax (new activations, the key is not touched in between): id, amax zero again, state, h_next"""
    t, te = getattr(O, tname), _embed_types(O)[ti]
    rng = np.random.default_rng(ti + K + n)
    packed = O.quantize(t, (rng.standard_normal((n, k)) * 0.05).astype(np.float32)).reshape(n, -1)
    keep, m = repack(be, O, t, packed, n, k)
    table, rows = make_table(O, te, n, K, seed=200 + ti)
    tb = be.buf(table)
    nw = np.abs(1.0 + 0.1 * rng.standard_normal(k)).astype(np.float32)
    nb = be.buf(nw) if norm else None
    st = DecodeState(be, 1, starts, step=2, stride=4)
    xb, out, h = be.buf(np.zeros(k, np.float32)), be.buf(np.full(n + 1, FSENT, np.float32)), be.buf(np.full((2, K), FSENT, np.float32))
    proj, adv = be.sym("mrs_dec_proj_argmax", PROJ_ARGMAX, C.c_int), be.sym("mrs_sample_advance_embed", ADV_EMBED, C.c_int)
    seen = []
    for call in range(3):  # tokens_out_stride 4 from step 2: written, written, dropped
        x = rng.standard_normal(k).astype(np.float32)
        xb.write(x)
        assert proj(C.byref(m), n, xb.ptr, k, nb.ptr if norm else None, 1e-5, out.ptr, n, st.ptr("scratch"), be.stream) == 0
        assert adv(*st.args(), tb.ptr, te, h.ptr, K, be.stream) == 0
        xe = O.rms_norm_engine(x[None], nw, 1e-5)[0] if norm else x
        logits = O.gemv_engine(t, packed, n, k, xe)[0]
        _bits_equal(out.numpy()[:n], logits, "engine-order oracle")
        tok = ref_argmax(logits)
        st.advance([tok])
        st.check()  # next_ids[0] == tok, amax zero again, positions / context_lens / slot_mapping / tokens_out / step_counter
        _bits_equal(h.numpy(), np.stack([rows[tok], np.full(K, FSENT, np.float32)]), ("h_next", te, K, tok))
        seen.append(tok)
    assert len(set(seen)) > 1, "the calls must not all choose the same id"


CHAIN = [(0, 256, "Q4_K", 33, 512, True, [30]), (1, 8448, "Q8_0", 257, 512, False, [31]), (2, 256, "Q6_K", 515, 512, True, [93]), (3, 8448, "Q4_K", 33, 512, True, [94]),
         (4, 8448, "Q5_K", 70, 768, True, [95]), (5, 8448, "Q6_K", 515, 512, True, [31]), (6, 8448, "Q8_0", 257, 512, False, [29]), (3, 256, "Q4_K", 1000, 1024, False, [96]),
         (4, 256, "Q5_K", 70, 768, True, [62]), (5, 256, "Q8_0", 257, 512, False, [0]), (6, 256, "Q4_K", 33, 512, True, [94])]


@pytest.mark.parametrize("ti,K,tname,n,k,norm,starts", [c for c in CHAIN if c[3] < 500 or c[0] == 5])  # (one of the 515-row heads; the emulation needs seconds per launch there)
def test_chain_host_emulation(oracle, ti, K, tname, n, k, norm, starts):
    check_chain(oracle, HostBackend(), ti, K, tname, n, k, norm, starts)


@pytest.mark.gpu
@pytest.mark.parametrize("ti,K,tname,n,k,norm,starts", CHAIN)
def test_chain_gpu(oracle, dev, ti, K, tname, n, k, norm, starts):
    check_chain(oracle, GpuBackend(dev), ti, K, tname, n, k, norm, starts)


def check_advance_embed_refusals(O, be):
    """NULL scratch, NULL table, NULL h_next, K <= 0 and type 2 (Q4_0) return -1 and touch nothing"""
    K = 256
    table, rows = make_table(O, O.Q4_K, 4, K, seed=1)
    tb, h = be.buf(table), be.buf(np.full((2, K), FSENT, np.float32))
    st = DecodeState(be, 1, [5], step=1)
    fn = be.sym("mrs_sample_advance_embed", ADV_EMBED, C.c_int)
    a = st.args()
    assert fn(*a[:-1], None, tb.ptr, O.Q4_K, h.ptr, K, be.stream) == -1
    assert fn(*a, None, O.Q4_K, h.ptr, K, be.stream) == -1
    assert fn(*a, tb.ptr, O.Q4_K, None, K, be.stream) == -1
    assert fn(*a, tb.ptr, O.Q4_K, h.ptr, 0, be.stream) == -1
    assert fn(*a, tb.ptr, O.Q4_K, h.ptr, -256, be.stream) == -1
    assert fn(*a, tb.ptr, T_Q4_0, h.ptr, K, be.stream) == -1
    st.check()
    assert (h.numpy() == FSENT).all()


def test_advance_embed_refusals_host_emulation(oracle):
    check_advance_embed_refusals(oracle, HostBackend())


@pytest.mark.gpu
def test_advance_embed_refusals_gpu(oracle, dev):
    check_advance_embed_refusals(oracle, GpuBackend(dev))


# ------------------------------------------------------------------------------------------------ 5. mrs_embedding
def check_embedding(O, be, ti, K):
    """K = 256: 8 slices, most threads idle; K = 8448: 264 slices, the slice loop takes a second pass.  Vocab 11, ids: last row, first row, repeats.  One guard row."""
    t = _embed_types(O)[ti]
    vocab, ids = 11, np.array([10, 0, 0, 7, 10], np.int32)
    table, rows = make_table(O, t, vocab, K, seed=300 + ti)
    tb, ib = be.buf(table), be.buf(ids)
    out = be.buf(np.full((len(ids) + 1, K), FSENT, np.float32))
    fn = be.sym("mrs_embedding", EMBED, C.c_int)
    assert fn(tb.ptr, t, ib.ptr, out.ptr, K, len(ids), be.stream) == 0
    _bits_equal(out.numpy(), np.concatenate([rows[ids], np.full((1, K), FSENT, np.float32)]), ("mrs_embedding", t, K))
    out.write(np.full((len(ids) + 1, K), FSENT, np.float32))
    assert fn(tb.ptr, t, ib.ptr, out.ptr, K, 0, be.stream) == -1       # tokens == 0
    assert fn(tb.ptr, T_Q4_0, ib.ptr, out.ptr, K, len(ids), be.stream) == -1  # a type without a row decoder here
    assert (out.numpy() == FSENT).all()


@pytest.mark.parametrize("K", [256, 8448])
@pytest.mark.parametrize("ti", range(7))
def test_embedding_host_emulation(oracle, ti, K):
    check_embedding(oracle, HostBackend(), ti, K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 8448])
@pytest.mark.parametrize("ti", range(7))
def test_embedding_gpu(oracle, dev, ti, K):
    check_embedding(oracle, GpuBackend(dev), ti, K)
