"""GPU: the MLA cache ops and paged_attn.flashinfer_mla_decode against an f64 reference that is the op's semantics taken literally.

Tolerance of the decode, derived (not measured).  `want` is the f64 result, `pabs` the same reference with |ckv| as values (it bounds every partial sum
the kernel forms), eps the unit roundoff of the tensor dtype (2^-8 bf16, 2^-11 f16).  The kernel rounds each un-normalised probability ONCE to the
dtype (eps * pabs) and the output once (eps * |want|).  A score is an f32 dot product of length 576 times the scale: |error| <= delta = (576 + 2) * 2^-24
* sm_scale * max_t sum_d |q||c|; it multiplies a key's weight by at most e^delta in the numerator and the denominator, so the normalised output moves by
at most (e^(2 delta) - 1) * pabs <= 2.5 delta * pabs.  exp and the f32 sums take the absolute term 1e-4 * max|ckv| of tests/test_zz_flash_attn_sinks_gpu.py.
Split partials stay f32, so splitting adds nothing.  tol = eps * pabs + eps * |want| + 2.5 * delta * pabs + 1e-4 * max|ckv|.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SCALE = 192 ** -0.5


def draw(rng, shape, dtype):
    return torch.from_numpy(rng.standard_normal(shape)).to(dtype)  # rounded through the tensor dtype: the reference sees the kernel's inputs


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
def test_cache_round_trip(dtype):
    from mistralrs_amd import paged_attn
    rng = np.random.default_rng(7)
    bs, nb, sentinel = 16, 4, -7.0
    table = torch.tensor([[2, 0, 1, 1], [3, 1, 1, 1]], dtype=torch.int32)  # block 1 is never written; the last columns are unused
    seq_lens = (20, 5)
    where = [(s, pos) for s, n in enumerate(seq_lens) for pos in range(n)]
    order = rng.permutation(len(where))  # input row j holds token where[order[j]]; one padding row (slot -1) goes in the middle
    slots = [int(table[where[i][0], where[i][1] // bs]) * bs + where[i][1] % bs for i in order]
    slots.insert(11, -1)
    T = len(slots)
    ckv_buf, kpe_buf = draw(rng, (T, 520), DT[dtype]).cuda(), draw(rng, (T, 68), DT[dtype]).cuda()
    ckv, kpe = ckv_buf[:, :512], kpe_buf[:, 2:66]  # row strides larger than the rows; the rotary rows start off a 16-byte boundary
    ckv_cache = torch.full((nb, bs, 512), sentinel, dtype=DT[dtype], device="cuda")
    kpe_cache = torch.full((nb, bs, 64), sentinel, dtype=DT[dtype], device="cuda")
    paged_attn.concat_and_cache_mla(ckv, kpe, ckv_cache, kpe_cache, torch.tensor(slots, dtype=torch.int64).cuda())
    cu = torch.tensor([0, 20, 25], dtype=torch.int32).cuda()
    t2s = torch.tensor([s for s, _ in where], dtype=torch.int32).cuda()
    g_ckv, g_kpe = paged_attn.gather_mla_cache(ckv_cache, kpe_cache, table.cuda(), cu, t2s)
    rows = [j for j in range(T) if slots[j] >= 0]  # input rows without the padding one, in the order of `order`
    back = torch.tensor(rows)[torch.from_numpy(np.argsort(order))]
    bits = torch.int32 if dtype == "f32" else torch.int16
    assert torch.equal(g_ckv.view(bits), ckv[back.cuda()].contiguous().view(bits))
    assert torch.equal(g_kpe.view(bits), kpe[back.cuda()].contiguous().view(bits))
    untouched = torch.ones(nb * bs, dtype=torch.bool)
    untouched[[s for s in slots if s >= 0]] = False
    assert untouched.sum() == nb * bs - 25
    assert (ckv_cache.view(nb * bs, 512)[untouched.cuda()] == sentinel).all() and (kpe_cache.view(nb * bs, 64)[untouched.cuda()] == sentinel).all()


DECODE = [  # dtype, heads, page size, request lengths, num_splits; "same" = the requests list the same pages (a speculative verify)
    ("bf16", 1, 16, (1, 0, 33), 1), ("bf16", 1, 32, (33, 1), 3), ("bf16", 16, 16, (200, 16, 0), 3), ("f16", 16, 32, (65, 33, 1), None),
    ("bf16", 40, 32, (65, 200), 1), ("f16", 40, 16, (33, 0, 16), 3), ("f16", 40, 32, (200, 65, 1), None), ("bf16", 128, 16, (200, 1), 3),
    ("f16", 128, 32, (65, 16), 1), ("bf16", 128, 32, (33, 200, 0), None), ("f16", 1, 16, (200,), 3), ("bf16", 16, 16, "same", None),
]


@pytest.mark.parametrize("dtype,heads,page,lens,splits", DECODE)
def test_decode(dtype, heads, page, lens, splits):
    from mistralrs_amd import paged_attn
    rng = np.random.default_rng(99)
    same = lens == "same"
    if same:
        lens = (198, 199, 200)
    B = len(lens)
    npages = [-(-n // page) for n in lens]
    free = rng.permutation((max(npages) if same else sum(npages)) + 2)  # shuffled page ids, two pages unused
    owned, at = [], 0
    for n in npages:
        owned.append(free[:n] if same else free[at:at + n])
        at += n
    indptr = np.concatenate([[0], np.cumsum(npages)]).astype(np.int32)
    indices = np.concatenate(owned + [np.zeros(0, np.int64)]).astype(np.int32)
    last = np.array([(n - 1) % page + 1 if n else 0 for n in lens], np.int32)
    ckv = torch.full((len(free), page, 512), float("nan"), dtype=DT[dtype])  # unused pages and rows past a request's end stay NaN
    kpe = torch.full((len(free), page, 64), float("nan"), dtype=DT[dtype])
    for b in np.argsort(lens):  # "same": the longest request fills the shared pages last, with fresh values for every row it owns
        flat = (owned[b][:, None] * page + np.arange(page)).reshape(-1)[:lens[b]]
        ckv.view(-1, 512)[flat] = draw(rng, (lens[b], 512), DT[dtype])
        kpe.view(-1, 64)[flat] = draw(rng, (lens[b], 64), DT[dtype])
    q_nope, q_pe = draw(rng, (B, heads, 512), DT[dtype]), draw(rng, (B, heads, 64), DT[dtype])
    out = paged_attn.flashinfer_mla_decode(q_nope.cuda(), q_pe.cuda(), ckv.cuda(), kpe.cuda(), *(torch.from_numpy(x).cuda() for x in (indptr, indices, last)),
                                           SCALE, num_splits=splits)
    assert out.shape == q_nope.shape and out.dtype == q_nope.dtype
    got, worst = out.double().cpu().numpy(), 0.0
    eps = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    for b in range(B):
        if lens[b] == 0:
            assert (got[b] == 0).all()
            continue
        flat = (owned[b][:, None] * page + np.arange(page)).reshape(-1)[:lens[b]]
        c, r = ckv.view(-1, 512)[flat].double().numpy(), kpe.view(-1, 64)[flat].double().numpy()
        qn, qp = q_nope[b].double().numpy(), q_pe[b].double().numpy()
        s = SCALE * (qn @ c.T + qp @ r.T)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        want, pabs = p @ c, p @ np.abs(c)
        delta = (576 + 2) * 2.0 ** -24 * SCALE * (np.abs(qn) @ np.abs(c).T + np.abs(qp) @ np.abs(r).T).max(-1, keepdims=True)
        tol = eps * pabs + eps * np.abs(want) + 2.5 * delta * pabs + 1e-4 * np.abs(c).max()
        err = np.abs(got[b] - want)
        assert np.isfinite(got[b]).all()
        worst = max(worst, (err / tol).max())
        assert (err <= tol).all()
    print(f"worst err / tol {worst:.3f}")


def test_checks_raise():
    from mistralrs_amd import paged_attn
    z = lambda *shape, dtype=torch.bfloat16: torch.zeros(*shape, dtype=dtype, device="cuda")
    meta = (torch.tensor([0, 1], dtype=torch.int32).cuda(), torch.tensor([0], dtype=torch.int32).cuda(), torch.tensor([1], dtype=torch.int32).cuda())
    with pytest.raises(ValueError):  # head dims other than 512 / 64
        paged_attn.flashinfer_mla_decode(z(1, 4, 256), z(1, 4, 64), z(2, 16, 256), z(2, 16, 64), *meta, SCALE)
    with pytest.raises(ValueError):  # f32 has no kernel
        f32 = torch.float32
        paged_attn.flashinfer_mla_decode(z(1, 4, 512, dtype=f32), z(1, 4, 64, dtype=f32), z(2, 16, 512, dtype=f32), z(2, 16, 64, dtype=f32), *meta, SCALE)
    with pytest.raises(ValueError):  # indptr must have batch + 1 entries
        paged_attn.flashinfer_mla_decode(z(1, 4, 512), z(1, 4, 64), z(2, 16, 512), z(2, 16, 64), meta[0][:1], meta[1], meta[2], SCALE)
