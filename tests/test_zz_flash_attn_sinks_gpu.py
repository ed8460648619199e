"""GPU: paged_attn.flash_attn_sinks / flash_attn_sinks_varlen against an f64 reference that is the op's semantics taken literally.

Tolerance, derived (not measured).  `want` is the f64 result, `pabs` the same reference run with |V| (the probability-weighted mean of |V|, which
bounds every partial sum the kernel forms), eps the unit roundoff of the tensor dtype (2^-8 bf16, 2^-11 f16).
  16-bit: the kernel rounds each un-normalised probability ONCE to the dtype (relative error <= eps per term, so <= eps * pabs on the output) and
  rounds the output once (eps * |want|); exp and the f32 sums are covered by the absolute term 1e-4 * max|V| that
  tests/test_paged_attn.py::test_prefill_attention uses.  tol = eps * pabs + eps * |want| + 1e-4 * max|V|.
  f32: nothing is rounded to 16 bits.  A score is an f32 dot product of length D times the scale: |error| <= delta = (D + 2) * 2^-24 * scale *
  sum|q||k| (we take the largest key of the row).  A score error delta multiplies that key's weight by at most e^delta, in the numerator and in
  the denominator, so the normalised output moves by at most (e^(2 delta) - 1) * pabs <= 2.5 delta * pabs for delta < 0.2; accumulating n <= 77
  products and the denominator in f32 adds (n + 2) * 2^-24 * pabs.  tol = (2.5 delta + 80 * 2^-24) * pabs + 1e-4 * max|V|.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def ref(q, k, v, sinks, scale, W):
    """one sequence, f64: q [H, ql, D], k / v [Hkv, kl, D] -> [H, ql, D]"""
    (H, ql, _), (Hkv, kl, _) = q.shape, k.shape
    out, off = np.zeros_like(q), kl - ql
    for h in range(H):
        g = h // (H // Hkv)
        for r in range(ql):
            hi = r + off
            lo = max(0, hi - W + 1) if W > 0 else 0
            if hi < 0:
                continue  # no visible key: zeros, with or without a sink
            s = scale * (k[g, lo:hi + 1] @ q[h, r])
            m = s.max() if sinks is None else max(s.max(), sinks[h])
            p = np.exp(s - m)
            l = p.sum() + (0.0 if sinks is None else np.exp(sinks[h] - m))
            out[h, r] = p @ v[g, lo:hi + 1] / l
    return out


def draw(rng, shape, dtype, mul=1.0):
    return (torch.from_numpy(rng.standard_normal(shape)) * mul).to(dtype)  # rounded through the tensor dtype: the reference sees the kernel's inputs


def tolerance(dtype, want, pabs, q, k, v, scale, kv_head_of):
    vmax = np.abs(v).max()
    if dtype != "f32":
        eps = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
        return eps * pabs + eps * np.abs(want) + 1e-4 * vmax
    D = q.shape[-1]
    sabs = np.einsum("hrd,hkd->hrk", np.abs(q), np.abs(k)[kv_head_of]).max(-1)  # [H, ql]
    delta = (D + 2) * 2.0 ** -24 * scale * sabs[..., None]
    return (2.5 * delta + 80 * 2.0 ** -24) * pabs + 1e-4 * vmax


def check(dtype, got, q, k, v, sinks, scale, W):
    """got, q [H, ql, D]; k, v [Hkv, kl, D]: one sequence, f64 numpy"""
    H, Hkv = q.shape[0], k.shape[0]
    want, pabs = ref(q, k, v, sinks, scale, W), ref(q, k, np.abs(v), sinks, scale, W)
    assert np.isfinite(got).all()
    tol = tolerance(dtype, want, pabs, q, k, v, scale, np.arange(H) // (H // Hkv))
    err = np.abs(got - want)
    print(f"max err {err.max():.3e}  max err/tol {(err / tol).max():.3f}")
    assert (err <= tol).all()
    dead = max(0, q.shape[1] - k.shape[1])  # rows with no visible key
    assert (got[:, :dead] == 0).all()


DENSE = [  # dtype, D, (H, Hkv), (q_len, kv_len), W, sinks
    ("bf16", 64, (8, 1), (70, 70), 48, "on"), ("bf16", 80, (4, 4), (1, 1), 0, None), ("bf16", 128, (6, 2), (33, 33), 5, "on"),
    ("bf16", 256, (4, 4), (33, 77), 0, "on"), ("bf16", 64, (6, 2), (40, 25), 5, None), ("bf16", 128, (8, 1), (33, 77), 48, None),
    ("bf16", 80, (6, 2), (70, 70), 0, "on"), ("bf16", 256, (8, 1), (40, 25), 48, "on"), ("bf16", 64, (4, 4), (33, 33), 48, None),
    ("bf16", 128, (4, 4), (70, 70), 5, "on"), ("bf16", 64, (4, 4), (33, 33), 0, "pm30"),
    ("f16", 256, (6, 2), (33, 77), 5, "on"), ("f16", 64, (8, 1), (70, 70), 48, None), ("f16", 80, (4, 4), (40, 25), 0, "on"),
    ("f16", 128, (6, 2), (1, 1), 48, None), ("f16", 64, (4, 4), (33, 33), 5, "on"), ("f16", 80, (8, 1), (33, 77), 0, None),
    ("f16", 128, (8, 1), (40, 25), 5, "on"), ("f16", 256, (4, 4), (70, 70), 48, None), ("f16", 64, (6, 2), (70, 70), 0, "on"),
    ("f16", 128, (4, 4), (33, 33), 0, None),
    ("f32", 80, (6, 2), (40, 25), 5, "on"), ("f32", 64, (8, 1), (70, 70), 48, "on"), ("f32", 128, (4, 4), (33, 33), 0, None),
    ("f32", 256, (6, 2), (33, 77), 48, None), ("f32", 64, (4, 4), (1, 1), 5, "on"), ("f32", 256, (8, 1), (70, 70), 5, None),
    ("f32", 128, (6, 2), (70, 70), 0, "on"), ("f32", 80, (4, 4), (33, 77), 48, "on"), ("f32", 256, (4, 4), (40, 25), 0, "on"),
    ("f32", 64, (6, 2), (33, 77), 0, None),
]


@pytest.mark.parametrize("dtype,D,heads,lens,W,sink_mode", DENSE)
def test_dense(dtype, D, heads, lens, W, sink_mode):
    from mistralrs_amd import paged_attn
    (H, Hkv), (ql, kl), B = heads, lens, 2
    rng = np.random.default_rng(1234)
    scale = D ** -0.5
    q, k, v = draw(rng, (B, H, ql, D), DT[dtype], 2.0), draw(rng, (B, Hkv, kl, D), DT[dtype]), draw(rng, (B, Hkv, kl, D), DT[dtype])
    sinks = None
    if sink_mode == "on":
        sinks = torch.from_numpy(rng.standard_normal(H) * 2).float()
    elif sink_mode == "pm30":  # the sink dominates head 0 and vanishes on head 1
        sinks = torch.tensor([30.0, -30.0] + [0.5] * (H - 2))
    out = paged_attn.flash_attn_sinks(q.cuda(), k.cuda(), v.cuda(), None if sinks is None else sinks.cuda(), scale, W)
    assert out.shape == q.shape and out.dtype == q.dtype
    got = out.double().cpu().numpy()
    sk = None if sinks is None else sinks.double().numpy()
    for b in range(B):
        check(dtype, got[b], q[b].double().numpy(), k[b].double().numpy(), v[b].double().numpy(), sk, scale, W)


@pytest.mark.parametrize("W", [0, 5])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_varlen(dtype, D, W):
    from mistralrs_amd import paged_attn
    H, Hkv, qls, kls, max_q = 8, 2, (1, 33, 20), (1, 50, 20), 40
    rng = np.random.default_rng(4321)
    scale = D ** -0.5
    q, k, v = draw(rng, (3, H, max_q, D), DT[dtype], 2.0), draw(rng, (sum(kls), Hkv, D), DT[dtype]), draw(rng, (sum(kls), Hkv, D), DT[dtype])
    sinks = torch.from_numpy(rng.standard_normal(H) * 2).float()
    cu = [torch.from_numpy(np.concatenate([[0], np.cumsum(x)]).astype(np.uint32)).cuda() for x in (qls, kls)]
    run = lambda vv: paged_attn.flash_attn_sinks_varlen(q.cuda(), k.cuda(), vv.cuda(), sinks.cuda(), cu[0], cu[1], scale, W)
    out = run(v)
    got = out.double().cpu().numpy()
    k0 = 0
    for b in range(3):
        kb, vb = (x[k0:k0 + kls[b]].transpose(0, 1).double().numpy() for x in (k, v))
        check(dtype, got[b][:, :qls[b]], q[b][:, :qls[b]].double().numpy(), kb, vb, sinks.double().numpy(), scale, W)
        assert (got[b][:, qls[b]:] == 0).all()  # padding rows come back as zeros
        k0 += kls[b]
    if dtype == "bf16" and D == 64:  # the neighbours' packed rows must not leak into sequence 1: poison them, same bits
        v2 = v.clone()
        v2[:kls[0]] = float("nan")
        v2[kls[0] + kls[1]:] = float("nan")
        assert torch.equal(run(v2)[1].view(torch.int16), out[1].view(torch.int16))


def test_checks_raise():
    from mistralrs_amd import paged_attn
    q = torch.zeros(1, 4, 8, 48, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        paged_attn.flash_attn_sinks(q, q, q, None, 1.0, 0)  # head size 48 is not in the list
