"""The FlashInfer-layout (HND) cache ops and paged_attn.flashinfer_decode against an f64 reference that is the op's semantics taken literally, computed
from the very tensors the kernel sees (inputs rounded through their dtype, E4M3 pages read back as float(code) * scale).

Tolerance of the decode, derived (not measured), as in tests/test_zz_mla_gpu.py.  `want` = p @ v in f64, `pabs` = p @ |v| (it bounds every partial sum the
kernel forms), eps the unit roundoff of the query dtype (2^-8 bf16, 2^-11 f16).  The kernel rounds each un-normalised probability ONCE to the dtype
(eps * pabs) and the output once (eps * |want|).  A score is an f32 dot product of length D times the scale: |error| <= delta = (D + 2) * 2^-24 * scale *
max_keys sum_d |q||k|; tanh is 1-Lipschitz, so the cap does not enlarge it, and the kernel's tanh is the library tanhf (a couple of ulps, not an
approximation: nothing is added for it).  delta moves a key's weight by at most e^delta in numerator and denominator: (e^(2 delta) - 1) * pabs <= 2.5 delta
* pabs.  exp and the f32 sums take the absolute term 1e-4 * max|v|.  Split partials are f32, so splitting adds nothing.
tol = eps * pabs + eps * |want| + 2.5 * delta * pabs + 1e-4 * max|v|, for every element.
"""
import numpy as np
import pytest
import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
F8 = torch.float8_e4m3fn


def draw(rng, shape, dtype):
    return torch.from_numpy(rng.standard_normal(shape)).to(dtype)  # rounded through the tensor dtype: the reference sees the kernel's inputs


@pytest.mark.gpu
@pytest.mark.parametrize("cache", ["same", "fp8"])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
def test_cache_round_trip(dtype, cache):
    from mistralrs_amd import paged_attn
    rng = np.random.default_rng(7)
    bs, nb, H, D, sentinel = 16, 4, 2, 64, -7.0
    ks, vs = (0.5, 2.0) if cache == "fp8" else (1.0, 1.0)
    table = torch.tensor([[2, 0, 1, 1], [3, 1, 1, 1]], dtype=torch.int32)  # block 1 is never written; the last columns are unused
    seq_lens = (20, 5)
    where = [(s, pos) for s, n in enumerate(seq_lens) for pos in range(n)]
    order = rng.permutation(len(where))  # input row j holds token where[order[j]]; one padding row (slot -1) goes in the middle
    slots = [int(table[where[i][0], where[i][1] // bs]) * bs + where[i][1] % bs for i in order]
    slots.insert(11, -1)
    T = len(slots)
    kbuf, vbuf = draw(rng, (T, H * D + 8), DT[dtype]).cuda(), draw(rng, (T, H * D + 8), DT[dtype]).cuda()
    key, value = kbuf[:, :H * D].view(T, H, D), vbuf[:, 2:H * D + 2].view(T, H, D)  # row strides larger than the rows; the value rows start off 16 bytes
    shape = paged_attn.flashinfer_cache_shape(nb, H, D, bs)
    assert shape == (nb, H, bs, D)
    cdt = F8 if cache == "fp8" else DT[dtype]
    kc, vc = (torch.full(shape, sentinel, dtype=torch.float32).to(cdt).cuda() for _ in range(2))
    paged_attn.reshape_and_cache_flashinfer(key, value, kc, vc, torch.tensor(slots, dtype=torch.int64).cuda(), ks, vs)
    cu = torch.tensor([0, 20, 25], dtype=torch.int32).cuda()
    gk, gv = paged_attn.gather_kv_cache_flashinfer(kc, vc, table.cuda(), cu, DT[dtype], ks, vs)
    rows = [j for j in range(T) if slots[j] >= 0]  # input rows without the padding one, in the order of `order`
    back = torch.tensor(rows)[torch.from_numpy(np.argsort(order))]
    bits = torch.int32 if dtype == "f32" else torch.int16
    for got, x, s in ((gk, key, ks), (gv, value, vs)):
        want = x.cpu()[back]
        if cache == "fp8":
            want = ((want.float() / s).to(F8).float() * s).to(DT[dtype])
        assert torch.equal(got.cpu().view(bits), want.contiguous().view(bits))
    untouched = torch.ones(nb, bs, dtype=torch.bool)
    untouched.view(-1)[[s for s in slots if s >= 0]] = False
    assert untouched.sum() == nb * bs - 25
    for c in (kc, vc):
        assert (c.cpu().float().permute(0, 2, 1, 3)[untouched] == sentinel).all()


DECODE = [  # dtype, cache, H, Hkv, D, page, request lengths ("same": three requests list the same pages), split_pages (None: partition=False), window, cap
    ("bf16", "same", 4, 1, 128, 16, (1, 0, 33), None, None, None), ("bf16", "same", 1, 1, 64, 16, (1, 0, 33), 1, None, None),
    ("f16", "same", 7, 1, 128, 32, (200, 65, 16), 3, None, None), ("bf16", "same", 32, 2, 128, 16, (200, 65, 16), 1, 20, None),
    ("f16", "same", 8, 2, 256, 16, (200, 65, 16), 3, None, 30.0), ("bf16", "fp8", 8, 2, 128, 32, (200, 65, 16), 3, None, None),
    ("f16", "fp8", 14, 2, 64, 16, "same", 1, 1000, 30.0), ("bf16", "same", 16, 1, 256, 32, "same", None, 0, None),
    ("bf16", "same", 16, 4, 64, 32, (200, 65, 16), None, 20, 30.0), ("f16", "same", 16, 1, 128, 16, (1, 0, 33), 3, 0, None),
    ("bf16", "same", 7, 7, 128, 16, "same", 3, 1000, None), ("f16", "same", 64, 4, 128, 32, (200, 65, 16), 1, None, None),
    ("bf16", "same", 28, 4, 256, 16, (1, 0, 33), 1, 20, None), ("f16", "same", 4, 1, 64, 32, "same", 3, 20, 30.0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,cache,H,Hkv,D,page,lens,split_pages,window_left,soft_cap", DECODE)
def test_decode(dtype, cache, H, Hkv, D, page, lens, split_pages, window_left, soft_cap):
    from mistralrs_amd import paged_attn
    rng = np.random.default_rng(99)
    same = lens == "same"
    if same:
        lens = (198, 199, 200)
    B, G, sm = len(lens), H // Hkv, D ** -0.5
    ks, vs = (0.5, 2.0) if cache == "fp8" else (1.0, 1.0)
    npages = [-(-n // page) for n in lens]
    free = rng.permutation((max(npages) if same else sum(npages)) + 2)  # shuffled page ids, two pages unused
    owned, at = [], 0
    for n in npages:
        owned.append(free[:n] if same else free[at:at + n])
        at += n
    indptr = np.concatenate([[0], np.cumsum(npages)]).astype(np.int32)
    indices = np.concatenate(owned + [np.zeros(0, np.int64)]).astype(np.int32)
    last = np.array([(n - 1) % page + 1 if n else 0 for n in lens], np.int32)
    kf, vf = (torch.full((len(free), Hkv, page, D), float("nan")) for _ in range(2))  # unused pages and rows past a request's end stay NaN
    at = [(torch.from_numpy(owned[b][np.arange(n) // page]), torch.arange(n) % page) for b, n in enumerate(lens)]
    for b in np.argsort(lens):  # "same": the longest request fills the shared pages last, with fresh values for every row it owns
        kf[at[b][0], :, at[b][1]] = draw(rng, (lens[b], Hkv, D), DT[dtype]).float() / ks
        vf[at[b][0], :, at[b][1]] = draw(rng, (lens[b], Hkv, D), DT[dtype]).float() / vs
    cdt = F8 if cache == "fp8" else DT[dtype]
    kc, vc = kf.to(cdt), vf.to(cdt)
    q = draw(rng, (B, H + 1, D + 8), DT[dtype])[:, :H, 4:D + 4]  # a slice of a wider buffer: both strides larger, rows 8 bytes off a 16-byte boundary
    tiles = int(paged_attn.flashinfer_decode_plan(lens, page, split_pages).o_indptr[-1])
    plan = paged_attn.flashinfer_decode_plan(lens, page, split_pages, tiles + 3, device="cuda")  # three padding tiles with mask 0
    out = paged_attn.flashinfer_decode(q.cuda(), kc.cuda(), vc.cuda(), *(torch.from_numpy(x).cuda() for x in (indptr, indices, last)), plan, sm,
                                       window_left=window_left, logits_soft_cap=soft_cap, k_scale=ks, v_scale=vs, partition=split_pages is not None)
    assert out.shape == (B, H, D) and out.dtype == DT[dtype]
    got, worst = out.double().cpu().numpy(), 0.0
    eps = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    kd, vd = kc.float().double() * ks, vc.float().double() * vs
    for b in range(B):
        if lens[b] == 0:
            assert (got[b] == 0).all()
            continue
        k, v = (np.repeat(x[at[b][0], :, at[b][1]].numpy(), G, axis=1) for x in (kd, vd))  # [len, H, D]
        qq = q[b].double().numpy()
        s = sm * np.einsum("hd,thd->ht", qq, k)
        if soft_cap is not None:
            s = soft_cap * np.tanh(s / soft_cap)
        if window_left is not None:
            s = np.where(np.arange(lens[b]) + 1 + window_left >= lens[b], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        want, pabs = np.einsum("ht,thd->hd", p, v), np.einsum("ht,thd->hd", p, np.abs(v))
        delta = (D + 2) * 2.0 ** -24 * sm * np.einsum("hd,thd->ht", np.abs(qq), np.abs(k)).max(-1, keepdims=True)
        tol = eps * pabs + eps * np.abs(want) + 2.5 * delta * pabs + 1e-4 * np.abs(v).max()
        assert np.isfinite(got[b]).all()
        err = np.abs(got[b] - want)
        worst = max(worst, (err / tol).max())
        assert (err <= tol).all()
    print(f"worst err / tol {worst:.3f}")


@pytest.mark.parametrize("split_pages,want", [
    (None, ([0, 1, 2, 3, 0, 0], [0, 0, 0, 0, 0, 0], [0, 1, 2, 3, 4], [16], [1, 1, 1, 1, 0, 0])),
    (3, ([0, 1, 2, 3, 3, 3, 3, 3, 0, 0], [0, 0, 0, 0, 1, 2, 3, 4, 0, 0], [0, 1, 2, 3, 8], [48], [1] * 8 + [0, 0])),
])
def test_plan(split_pages, want):  # lens 0 / 1 / 33 / 200 at page 16 are 0 / 1 / 3 / 13 pages; a request without a page still gets one tile
    from mistralrs_amd import paged_attn
    plan = paged_attn.flashinfer_decode_plan((0, 1, 33, 200), 16, split_pages, len(want[0]))
    assert [t.tolist() for t in plan] == list(want)
    assert [t.dtype for t in plan] == [torch.int32] * 4 + [torch.uint8]
    with pytest.raises(ValueError):
        paged_attn.flashinfer_decode_plan((0, 1, 33, 200), 16, split_pages, sum(want[4]) - 1)


@pytest.mark.gpu
def test_checks_raise():
    from mistralrs_amd import paged_attn
    bf16 = torch.bfloat16
    z = lambda *shape, dtype=bf16: torch.zeros(*shape, dtype=dtype, device="cuda")
    csr = tuple(torch.tensor(x, dtype=torch.int32).cuda() for x in ([0, 1], [0], [1]))
    plan = paged_attn.flashinfer_decode_plan((1,), 16, device="cuda")
    slots = torch.zeros(1, dtype=torch.int64).cuda()
    decode = lambda q, kc, plan=plan, csr=csr, **kw: paged_attn.flashinfer_decode(q, kc, kc.clone(), *csr, plan, 1.0, **kw)
    decode(z(1, 4, 64), z(2, 2, 16, 64))  # the base case is served
    for bad in (
        lambda: decode(z(1, 4, 64), z(2, 2, 16, 64, dtype=torch.float16)),  # a cache of another non-FP8 dtype
        lambda: decode(z(1, 4, 64), z(2, 2, 16, 64), k_scale=0.5),  # a non-unit scale with a bf16 cache
        lambda: decode(z(1, 4, 64), z(2, 2, 16, 64).to(F8), v_scale=0.0),  # a non-positive scale
        lambda: decode(z(1, 4, 64), z(2, 2, 16, 64), plan=plan._replace(kv_tile_indices=plan.kv_tile_indices.long())),  # plan dtype
        lambda: decode(z(1, 4, 64), z(2, 2, 16, 64), plan=plan._replace(block_valid_mask=z(2, dtype=torch.uint8))),  # plan length
        lambda: decode(z(1, 4, 64), z(2, 3, 16, 64)),  # H % Hkv != 0
        lambda: decode(z(1, 4, 64, dtype=torch.float32), z(2, 2, 16, 64, dtype=torch.float32)),  # refused: f32 queries
        lambda: decode(z(1, 4, 512), z(2, 2, 16, 512)),  # refused: head_size 512
        lambda: decode(z(1, 17, 64), z(2, 1, 16, 64)),  # refused: more than 16 heads per KV head
        lambda: decode(z(1, 4, 64), z(2, 2, 8, 64)),  # refused: another page size
        lambda: paged_attn.reshape_and_cache_flashinfer(z(1, 2, 64), z(1, 2, 64), z(2, 2, 16, 64), z(2, 2, 16, 64), slots.int()),  # i32 slots
        lambda: paged_attn.reshape_and_cache_flashinfer(z(1, 2, 64), z(1, 2, 64), z(2, 2, 16, 64), z(2, 2, 16, 64), slots, 2.0, 1.0),
        lambda: paged_attn.gather_kv_cache_flashinfer(z(2, 2, 16, 64), z(2, 2, 16, 32), csr[1].view(1, 1), csr[0], bf16),  # cache shapes differ
    ):
        with pytest.raises(ValueError):
            bad()
