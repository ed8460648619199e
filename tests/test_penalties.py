"""Penalties and logit bias for all rows of a step in one launch (csrc/sampling.hip, `mrs_penalties_f32_batched`), pinned BIT FOR BIT to the chain of single-row launches
the library already exports and tests (tests/test_sampling.py): apply_sparse_penalties_f32(generated counts, f, p, 1) -> apply_sparse_penalties_f32(all counts, 0, 0, rp)
-> apply_sparse_logits_bias_f32.  Bodies take a backend of tests/abi_backends.py -- the host emulation in the CPU suite, the MI355X under `-m gpu`.

The hand case pins the two facts the chain alone cannot: frequency and presence count GENERATED tokens only, repetition spans the prompt too."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

VP, I, F, LL = C.c_void_p, C.c_int, C.c_float, C.c_int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "mrs_penalties_f32_batched"
TRIPLES = [(0.3, 0.1, 1.0), (0.0, 0.0, 1.3), (0.7, -0.2, 0.8)]  # (frequency, presence, repetition): the triples of tests/test_sampling.py
EXACT_TRIPLES = [(0.001, 7.9, 1.1), (1.7, 0.0, 0.9), (-0.25, 0.0625, 2.0)]  # f and p are 0 or in [2^-10, 8]: penalties_host's float64 sum is exact
EDGES = [0, 2047, 2048, 4095, 4096, 5002]
SENTINEL = np.float32(-77.25)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def launch(be, x, contexts, prompt_lens, triples, biases, chunk, dst=None, nrows=None, ncols=None, pad=0):
    """one batched launch over `x` [rows, n]; biases: a list of (ids, values) per row, or None (bias_offsets == NULL); dst="in-place": x's own buffer is the output.
    Returns the whole output buffer as a flat array of rows * n + pad floats (the pad prefilled with SENTINEL)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, n = x.shape
    tok = np.concatenate([np.asarray(c, np.uint32) for c in contexts] + [np.zeros(1, np.uint32)])
    off = np.concatenate([[0], np.cumsum([len(c) for c in contexts])]).astype(np.int32)
    if dst == "in-place":
        xb = out = be.buf(np.concatenate([x.reshape(-1), np.full(pad, SENTINEL, np.float32)]))
    else:
        xb, out = be.buf(x), be.buf(np.full(rows * n + pad, SENTINEL, np.float32))
    tb, ob, pb = be.buf(tok), be.buf(off), be.buf(np.asarray(prompt_lens, np.int32))
    fb, qb, rb = (be.buf(np.asarray([t[j] for t in triples], np.float32)) for j in range(3))
    if biases is None:
        bi = bv = bo = None
    else:
        bi = be.buf(np.concatenate([np.asarray(b[0], np.uint32) for b in biases] + [np.zeros(1, np.uint32)]))
        bv = be.buf(np.concatenate([np.asarray(b[1], np.float32) for b in biases] + [np.zeros(1, np.float32)]))
        bo = be.buf(np.concatenate([[0], np.cumsum([len(b[0]) for b in biases])]).astype(np.int32))
    ptr = lambda b: None if b is None else b.ptr
    be.sym(SYM, [VP] * 11 + [I, I, I, LL])(xb.ptr, out.ptr, tb.ptr, ob.ptr, pb.ptr, fb.ptr, qb.ptr, rb.ptr, ptr(bi), ptr(bv), ptr(bo), rows if nrows is None else nrows,
                                          n if ncols is None else ncols, chunk, be.stream or 0)
    return out.numpy().reshape(-1).astype(np.float32)


def chain(be, x, context, prompt_len, triple, bias):
    """the expected row: the three existing single-row launches of the same backend, counts from a dict"""
    n = x.size
    f, p, rp = triple
    pen = be.sym("apply_sparse_penalties_f32", [VP, VP, VP, VP, I, I, F, F, F, LL])

    def counted(tokens):
        d = {}
        for t in tokens:
            d[int(t)] = d.get(int(t), 0) + 1
        return be.buf(np.array(list(d) + [0], np.uint32)), be.buf(np.array(list(d.values()) + [0], np.float32)), len(d)

    gen = context[min(prompt_len, len(context)):]
    cur = be.buf(np.ascontiguousarray(x, dtype=np.float32))
    for tokens, args in ((gen, (f, p, 1.0)), (context, (0.0, 0.0, rp))):
        ids, cnt, k = counted(tokens)
        nxt = be.buf(np.zeros(n, np.float32))
        pen(cur.ptr, nxt.ptr, ids.ptr, cnt.ptr, n, k, *args, be.stream or 0)
        cur = nxt
    out = be.buf(np.zeros(n, np.float32))
    ids, vals = be.buf(np.r_[np.asarray(bias[0], np.uint32), np.zeros(1, np.uint32)]), be.buf(np.r_[np.asarray(bias[1], np.float32), np.zeros(1, np.float32)])
    be.sym("apply_sparse_logits_bias_f32", [VP, VP, VP, VP, I, I, LL])(cur.ptr, out.ptr, ids.ptr, vals.ptr, n, len(bias[0]), be.stream or 0)
    return out.numpy().reshape(-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows_for(n, seed=3):
    """the four rows of body 1 for a vocabulary of n: (logits [4, n], contexts, prompt lengths, bias lists).  Row 0: empty context; row 1: 300 tokens, one id 40 times,
    ids on every chunk edge of n = 5003 at chunk 2048, ids >= n, prompt_len 120; row 2: the same tokens, prompt_len 0; row 3: prompt_len = len (nothing generated)."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((4, n)) * 4).astype(np.float32)
    x[1, 0] = -0.0
    hot = min(1234, n - 1)
    t = np.concatenate([EDGES, [hot] * 40, g.integers(0, n + 50, 300 - 40 - len(EDGES)), ]).astype(np.int64)
    t = t[g.permutation(t.size)]
    t[[10, 150]] = [n, n + 49]  # ids >= n in the prompt part and in the generated part
    ctx = [[], t.tolist(), t.tolist(), t[::-1].tolist()]
    assert len(ctx[1]) == 300 and ctx[1].count(hot) >= 40
    pls = [0, 120, 0, 300]
    bid = g.permutation(n + 20)[:40]
    bid = np.unique(np.concatenate([bid, [i for i in (2047, 2048, 4096, 5002) if i < n + 20]]))
    biases = [(np.array([min(2048, n - 1), n + 3], np.uint32), np.array([0.5, 9.0], np.float32)),  # on a chunk boundary, and one id >= n; the row's context is empty
              (bid.astype(np.uint32), g.standard_normal(bid.size).astype(np.float32)),
              (np.zeros(0, np.uint32), np.zeros(0, np.float32)),
              (np.array([0, hot] if hot else [0], np.uint32), np.array([-2.5, 0.0] if hot else [-2.5], np.float32))]
    x.setflags(write=False)
    return x, ctx, pls, biases


# ---------------------------------------------------------------- 1. chain equality, bitwise
CHAIN_CASES = [(5003, 2048, "plain"), (5003, 2048, "null-bias"), (5003, 2048, "in-place"), (1, 2048, "plain"), (2048, 2048, "plain"), (5003, 100, "plain")]


def check_chain(be, n, chunk, form):
    x, ctx, pls, biases = rows_for(n)
    none = [(np.zeros(0, np.uint32), np.zeros(0, np.float32))] * 4
    for shift in range(3):  # every triple meets every row
        triples = [TRIPLES[(r + shift) % 3] for r in range(4)]
        for pl3 in (pls[3], pls[3] + 7):  # prompt_len == len and prompt_len > len: nothing is generated either way
            lens = pls[:3] + [pl3]
            got = launch(be, x, ctx, lens, triples, None if form == "null-bias" else biases, chunk, dst="in-place" if form == "in-place" else None).reshape(4, n)
            for r in range(4):
                want = chain(be, x[r], ctx[r], lens[r], triples[r], none[r] if form == "null-bias" else biases[r])
                np.testing.assert_array_equal(u32(got[r]), u32(want), err_msg=f"row {r} n={n} chunk={chunk} {form} triples {triples[r]}")
    # the launch did something: row 1 differs from its input, row 0 only where its bias is
    assert (u32(got[1]) != u32(x[1])).sum() > 0 or n == 1
    if form == "null-bias":
        np.testing.assert_array_equal(u32(got[0]), u32(x[0]))  # an empty context and no bias: a plain copy


# ---------------------------------------------------------------- 2. the hand case
def check_hand_case(be):
    x = np.array([[1, -1, 2, -2, 4, -4, 8, -8]], np.float32)
    ctx = [[5, 5, 7] + [7, 9 % 8, 7]]
    bias = [(np.array([3, 5], np.uint32), np.array([1.5, -1.0], np.float32))]
    # token 1: generated once, negative: (-1 - (1 * 0.5 + 0.25)) * 2;  token 3: bias only;  token 5: in the PROMPT only -- no frequency / presence, repetition yes:
    # -4 * 2 - 1;  token 7: generated twice (and once in the prompt): (-8 - (2 * 0.5 + 0.25)) * 2
    want = np.array([1.0, -3.5, 2.0, -0.5, 4.0, -9.0, 8.0, -18.5], np.float32)
    for chunk in (2048, 3):
        got = launch(be, x, ctx, [3], [(0.5, 0.25, 2.0)], bias, chunk)
        np.testing.assert_array_equal(u32(got), u32(want))
    # positive logits are DIVIDED: the same context on the negated row, no bias
    got = launch(be, -x, ctx, [3], [(0.5, 0.25, 2.0)], None, 2048)
    np.testing.assert_array_equal(u32(got), u32(np.array([-1.0, 0.125, -2.0, 2.0, -4.0, 2.0, -8.0, 3.375], np.float32)))


# ---------------------------------------------------------------- 3. the host rule
def check_host_rule(be, n=5003, chunk=2048):
    from mistralrs_amd import sampler
    x, ctx, pls, biases = rows_for(n)
    for shift in range(3):
        triples = [EXACT_TRIPLES[(r + shift) % 3] for r in range(4)]
        got = launch(be, x, ctx, pls, triples, biases, chunk).reshape(4, n)
        for r in range(4):
            want = sampler.penalties_host(x[r], ctx[r], pls[r], *triples[r], {int(i): float(v) for i, v in zip(*biases[r])})
            np.testing.assert_array_equal(u32(got[r]), u32(want), err_msg=f"row {r} {triples[r]}")


# ---------------------------------------------------------------- 4. isolation and determinism
def check_isolation(be, n=5003, chunk=2048):
    x, ctx, pls, biases = rows_for(n)
    triples = [TRIPLES[r % 3] for r in range(4)]
    pad = n + 64
    first = launch(be, x, ctx, pls, triples, biases, chunk, pad=pad)
    again = launch(be, x, ctx, pls, triples, biases, chunk, pad=pad)
    assert first.size == 4 * n + pad
    np.testing.assert_array_equal(u32(first[4 * n:]), u32(np.full(pad, SENTINEL)))  # one row and 64 floats beyond the output: untouched
    np.testing.assert_array_equal(u32(first), u32(again))
    inplace = launch(be, x, ctx, pls, triples, biases, chunk, dst="in-place", pad=pad)
    np.testing.assert_array_equal(u32(inplace), u32(first))
    for r in range(4):
        alone = launch(be, x[r:r + 1], ctx[r:r + 1], pls[r:r + 1], triples[r:r + 1], biases[r:r + 1], chunk)
        np.testing.assert_array_equal(u32(alone), u32(first[r * n:(r + 1) * n]), err_msg=f"row {r} alone")
    # rows past nrows are not touched; nrows <= 0, ncols <= 0 and a chunk_size outside 1..4096 launch nothing
    two = launch(be, x, ctx, pls, triples, biases, chunk, nrows=2)
    np.testing.assert_array_equal(u32(two[:2 * n]), u32(first[:2 * n]))
    assert np.all(two[2 * n:] == SENTINEL)
    for kw in (dict(nrows=0), dict(nrows=-1), dict(ncols=0), dict(ncols=-5)):
        assert np.all(launch(be, x, ctx, pls, triples, biases, chunk, **kw) == SENTINEL), kw
    for bad in (0, -1, 4097):
        assert np.all(launch(be, x, ctx, pls, triples, biases, bad) == SENTINEL), bad


# ---------------------------------------------------------------- the backends
@pytest.fixture(scope="module")
def host():
    from tests.abi_backends import HostBackend
    return HostBackend()


@pytest.fixture(scope="module")
def gpu(dev):
    from tests.abi_backends import GpuBackend
    return GpuBackend(dev)


CHAIN_IDS = [f"n{c[0]}c{c[1]}{c[2]}" for c in CHAIN_CASES]


@pytest.mark.parametrize("n,chunk,form", CHAIN_CASES, ids=CHAIN_IDS)
def test_chain_equality_host_emulation(host, n, chunk, form):
    check_chain(host, n, chunk, form)


def test_hand_case_host_emulation(host):
    check_hand_case(host)


def test_host_rule_host_emulation(host):
    check_host_rule(host)


def test_isolation_and_determinism_host_emulation(host):
    check_isolation(host)


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunk,form", CHAIN_CASES, ids=CHAIN_IDS)
def test_chain_equality_gpu(gpu, n, chunk, form):
    check_chain(gpu, n, chunk, form)


@pytest.mark.gpu
def test_hand_case_gpu(gpu):
    check_hand_case(gpu)


@pytest.mark.gpu
def test_host_rule_gpu(gpu):
    check_host_rule(gpu)


@pytest.mark.gpu
def test_isolation_and_determinism_gpu(gpu):
    check_isolation(gpu)


# ---------------------------------------------------------------- 5. refusals of sampler.Penalties (construction and call validation: no launch, no GPU)
def test_penalties_class_refusals():
    import torch
    from mistralrs_amd import sampler
    cpu = torch.device("cpu")
    for args, kw in (((0, cpu), {}), ((97, cpu), dict(max_rows=0)), ((97, cpu), dict(max_rows=65536)), ((97, cpu), dict(max_context=-1))):
        with pytest.raises(ValueError, match=r"^penalties: "):
            sampler.Penalties(*args, **kw)
    pen = sampler.Penalties(97, cpu, max_rows=2, max_context=10)
    x = torch.zeros(2, 97)
    ctx = [[1, 2, 3], [4]]
    colon = [dict(frequency_penalty=float("nan")), dict(presence_penalty=float("inf")), dict(repetition_penalty=float("nan")), dict(frequency_penalty=1e39),
             dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5), dict(repetition_penalty=[1.0, 0.0]),
             dict(logit_bias={-1: 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={3: float("nan")}), dict(logit_bias=[None, {3: float("inf")}]), dict(logit_bias={3: 1e39})]
    for kw in colon:
        with pytest.raises(ValueError, match=r"^penalties: "):
            pen(x, ctx, 1, **kw)
    for bad_ctx in ([[1, -2, 3], [4]], [[1, 2.5], [4]], [[1, 2, 3], [float("nan")]], [list(range(8)), [1, 2, 3]]):  # the last: 11 tokens > max_context = 10
        with pytest.raises(ValueError, match=r"^penalties: "):
            pen(x, bad_ctx, 1)
    requires = [((x, [[1, 2, 3]], 1), {}), ((x, [1, 2], 1), {}), ((x, ctx, [1, 2, 3]), {}), ((x, ctx, -1), {}), ((x, ctx, 1.5), {}),
                ((x, ctx, 1), dict(frequency_penalty=[0.1, 0.2, 0.3])), ((x, ctx, 1), dict(logit_bias=[{1: 1.0}])), ((x, ctx, 1), dict(logit_bias=[(1, 1.0), None])),
                ((x, ctx, 1), dict(logit_bias={i: 1.0 for i in range(sampler.MAX_BIAS + 1)}))]
    for args, kw in requires:
        with pytest.raises(ValueError, match=r"^penalties requires "):
            pen(*args, **kw)
    for bad_x in (torch.zeros(3, 97), torch.zeros(2, 97, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"^penalties: logits"):
            pen(bad_x, ctx, 1)
    # penalties_host refuses the same values; penalties_active
    for kw in (dict(frequency_penalty=float("nan")), dict(repetition_penalty=0.0), dict(logit_bias={-1: 1.0}), dict(logit_bias={1: float("inf")})):
        with pytest.raises(ValueError, match=r"^penalties: "):
            sampler.penalties_host(np.zeros(97, np.float32), [1, 2], 1, **kw)
    with pytest.raises(ValueError, match=r"^penalties: "):
        sampler.penalties_host(np.zeros(97, np.float32), [1, -2], 1)
    act = sampler.penalties_active
    assert [act(None, None, None, None), act(0.0, 0.0, 1.0, {}), act(0.0, 0.0, 1.0, {5: 0.0}), act(0, 0, 1, None)] == [False] * 4
    assert all([act(0.1, None, None, None), act(None, -0.5, None, None), act(None, None, 1.1, None), act(0.0, 0.0, 1.0, {5: 0.0, 6: -1.0}), act(float("nan"), 0, 1, None)])
    # entries equal to 0 or with an id >= the vocabulary are dropped on the host: the row is left alone
    row = np.arange(8, dtype=np.float32) - 3
    np.testing.assert_array_equal(u32(sampler.penalties_host(row, [], 0, logit_bias={2: 0.0, 8: 5.0, 100: 1.0})), u32(row))


# ---------------------------------------------------------------- 6. the wrapper at a model's size
@pytest.mark.gpu
def test_penalties_class_at_vocabulary_size_gpu(dev):
    """8 rows x 128256 logits, contexts of 4000 tokens over 600 distinct ids, through sampler.Penalties (its packing included) against penalties_host, bitwise"""
    import torch
    from mistralrs_amd import sampler
    n, rows = 128256, 8
    g = np.random.default_rng(11)
    x = (g.standard_normal((rows, n)) * 4).astype(np.float32)
    ids = g.permutation(n + 100)[:600]
    ctx = [ids[g.integers(0, 600, 4000)].tolist() for _ in range(rows)]
    ctx[5] = []
    pls = [0, 1000, 4000, 3999, 2000, 0, 5000, 17]
    tri = [EXACT_TRIPLES[r % 3] for r in range(rows)]
    bias = [None if r % 3 == 0 else {int(i): float(np.float32(v)) for i, v in zip(g.permutation(n + 10)[:50 * r], g.standard_normal(50 * r))} for r in range(rows)]
    pen = sampler.Penalties(n, dev, max_rows=rows, max_context=4000 * rows)
    xt = torch.from_numpy(x).to(dev)
    got = pen(xt, ctx, pls, [t[0] for t in tri], [t[1] for t in tri], [t[2] for t in tri], bias).cpu().numpy()
    assert np.array_equal(xt.cpu().numpy().view(np.uint32), x.view(np.uint32))  # the input is left as it is
    for r in range(rows):
        want = sampler.penalties_host(x[r], ctx[r], pls[r], *tri[r], bias[r])
        np.testing.assert_array_equal(u32(got[r]), u32(want), err_msg=f"row {r}")
        assert r == 5 or (u32(got[r]) != u32(x[r])).sum() > 100
    # one row, scalars, one bias dict for all
    one = pen(xt[3], [ctx[3]], pls[3], 0.5, 0.25, 1.25, {7: 2.0, n + 1: 1.0}).cpu().numpy()
    np.testing.assert_array_equal(u32(one[0]), u32(sampler.penalties_host(x[3], ctx[3], pls[3], 0.5, 0.25, 1.25, {7: 2.0})))


# ---------------------------------------------------------------- 7. resources of the compiled kernel (no GPU)
def test_penalties_kernel_no_scratch_no_spills():
    lib = os.path.join(ROOT, "mistral.rs_amd", "lib", "libmistralrscuda.so")
    if not os.path.exists(lib):
        pytest.skip("libmistralrscuda.so not built (python mistral.rs_amd/build.py)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    ks = [k for k in m.resources(lib) if "penalties_batched_kernel" in k["demangled"] or "penalties_batched_kernel" in k["name"]]
    assert len(ks) == 1, [k["name"] for k in ks]
    k = ks[0]
    assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k
