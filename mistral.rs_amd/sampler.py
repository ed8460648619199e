"""Sampling: the roles of `Sampler::sample_topk_on_device` (mistralrs-core/src/sampler.rs:1171-1290) and of the batched device categorical draw
(pipeline/sampling.rs:999-1018, sampler.rs:649-652, 744-764).

With top-k set -- device half (csrc/sampling.hip, reference ABI `topk_large_f32_packed[_batched]`, ops.rs:691-1000): the k largest logits of a row in (value
descending, index ascending) order + the pieces of the full-softmax normaliser, ONE small device -> host copy of `2k + 2` floats per row.  Host half (this file):
probabilities of the candidates under the FULL softmax, the top-p cut, the min-p cut, the weighted draw.
Without top-k (temperature only, top-p and min-p inactive) -- the draw itself runs on the device (`categorical_large_f32_packed_batched`, ops.rs:1347-1500): the
cumulative distribution of softmax(x / T) is inverted at one uniform per row, and 2 floats per row (token, logprob) come back.  `categorical_host` states the same rule in
numpy f32; it serves logits that live on the CPU.
The reference draws with `rand`'s Isaac64Rng (+ WeightedIndex for top-k); this module draws with numpy's Generator from the SAME weights -- `uniform_for` for the
categorical path -- so the distribution is the reference's and the random stream is not (documented in DESIGN.md)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

CHUNK_SIZE = 2048      # CUDA_TOPK_CHUNK_SIZE (ops.rs:12)
MAX_K = 128            # CUDA_TOPK_MAX_K (ops.rs:18)
MAX_STAGE2 = 47 * 1024  # CUDA_TOPK_MAX_STAGE2_CANDIDATES (ops.rs:20)


class TopK:
    """Workspace + launcher for rows of `vocab` f32 logits (cuda_topk_logits_f32_packed / _batched, ops.rs:691-1000)."""

    def __init__(self, vocab: int, k: int, device, max_rows: int = 1):
        k = min(int(k), int(vocab))
        if vocab <= 0:
            raise ValueError("top-k: empty logits")
        if k == 0 or k > MAX_K:
            raise ValueError(f"top-k: k={k} must be in [1, {MAX_K}]")
        self.vocab, self.k, self.max_rows, self.device = vocab, k, max_rows, device
        self.nblocks = (vocab + CHUNK_SIZE - 1) // CHUNK_SIZE
        if self.nblocks * k > MAX_STAGE2:
            raise ValueError(f"top-k workspace too large: {self.nblocks * k} candidates")
        f32 = dict(dtype=torch.float32, device=device)
        self.block_values = torch.empty(max_rows, self.nblocks, k, **f32)
        self.block_indices = torch.empty(max_rows, self.nblocks, k, dtype=torch.int32, device=device)
        self.block_maxes = torch.empty(max_rows, self.nblocks, **f32)
        self.block_sums = torch.empty(max_rows, self.nblocks, **f32)
        self.packed = torch.empty(max_rows, 2 * k + 2, **f32)
        self._inv_t = torch.empty(max_rows, **f32)
        vp, i, f, ll = C.c_void_p, C.c_int, C.c_float, C.c_int64
        self._one = _lib.sym("core", "topk_large_f32_packed", [vp, vp, vp, vp, vp, vp, i, i, i, i, f, ll])
        self._many = _lib.sym("core", "topk_large_f32_packed_batched", [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, ll])

    def __call__(self, logits: torch.Tensor, temperature) -> torch.Tensor:
        """logits f32 [vocab] or [rows, vocab] (contiguous, on the device); temperature: a positive finite float, or one per row.  Returns the packed rows
        [rows, 2k + 2] on the device (a view of this object's buffer: consume it before the next call)."""
        x = logits.reshape(-1, self.vocab) if logits.dim() > 1 else logits.reshape(1, self.vocab)
        rows = x.shape[0]
        if x.dtype != torch.float32 or not x.is_contiguous() or rows > self.max_rows:
            raise ValueError("top-k: logits must be contiguous f32 with at most max_rows rows")
        temps = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (rows,))
        if not np.all(np.isfinite(temps) & (temps > 0)):
            raise ValueError("top-k requires a positive finite temperature")
        st = torch.cuda.current_stream().cuda_stream
        if rows == 1:
            self._one(x.data_ptr(), self.block_values.data_ptr(), self.block_indices.data_ptr(), self.block_maxes.data_ptr(), self.block_sums.data_ptr(),
                      self.packed.data_ptr(), self.vocab, self.k, CHUNK_SIZE, self.nblocks, float(np.float32(1.0 / temps[0])), st)
        else:
            self._inv_t[:rows].copy_(torch.from_numpy((1.0 / temps).astype(np.float32)), non_blocking=False)
            self._many(x.data_ptr(), self._inv_t.data_ptr(), self.block_values.data_ptr(), self.block_indices.data_ptr(), self.block_maxes.data_ptr(),
                       self.block_sums.data_ptr(), self.packed.data_ptr(), rows, self.vocab, self.k, CHUNK_SIZE, self.nblocks, st)
        return self.packed[:rows]


class Top1:
    """Greedy rows: `top1_large_f32_packed[_batched]` (cuda_top1_logits_f32_*, ops.rs:1232-2050) -- packed [rows][2] = (max logit, token id as f32); no temperature."""

    def __init__(self, vocab: int, device, max_rows: int = 1):
        if vocab <= 0:
            raise ValueError("top-1: empty logits")
        self.vocab, self.max_rows, self.device = vocab, max_rows, device
        self.nblocks = (vocab + CHUNK_SIZE - 1) // CHUNK_SIZE
        self.block_values = torch.empty(max_rows, self.nblocks, dtype=torch.float32, device=device)
        self.block_indices = torch.empty(max_rows, self.nblocks, dtype=torch.int32, device=device)
        self.packed = torch.empty(max_rows, 2, dtype=torch.float32, device=device)
        vp, i, ll = C.c_void_p, C.c_int, C.c_int64
        self._many = _lib.sym("core", "top1_large_f32_packed_batched", [vp, vp, vp, vp, vp, i, i, i, i, ll])

    def __call__(self, logits: torch.Tensor) -> torch.Tensor:
        x = logits.reshape(-1, self.vocab)
        rows = x.shape[0]
        if x.dtype != torch.float32 or not x.is_contiguous() or rows > self.max_rows:
            raise ValueError("top-1: logits must be contiguous f32 with at most max_rows rows")
        self._many(x.data_ptr(), self.block_values.data_ptr(), self.block_indices.data_ptr(), self.packed.data_ptr(), None, rows, self.vocab, CHUNK_SIZE, self.nblocks,
                   torch.cuda.current_stream().cuda_stream)
        return self.packed[:rows]


def top1_token(packed2) -> int:
    """Sampler::cuda_top1_token (sampler.rs:1284-1297): the packed pair must be finite and hold a non-negative integer"""
    mx, ix = float(packed2[0]), float(packed2[1])
    if not (np.isfinite(mx) and np.isfinite(ix)) or ix < 0 or ix != np.floor(ix):
        raise ValueError(f"invalid CUDA top-1 output: max_logit={mx} argmax={ix}")
    return int(ix)


def filtered_probs(packed: np.ndarray, k: int, temperature: float, top_p: float = 1.0, min_p: float = 0.0):
    """sampler.rs:1189-1236 for one packed row: (token ids [k], reporting probabilities [k], weights after the top-p and min-p cuts [k]); f32 like the reference."""
    vals, ids = packed[:k].astype(np.float32), packed[k:2 * k].astype(np.uint32)
    denom, gmax = np.float32(packed[2 * k]), np.float32(packed[2 * k + 1])
    if not (denom > 0 and np.isfinite(denom) and np.isfinite(gmax)):
        raise ValueError("invalid top-k softmax normalizer")
    inv_t = np.float32(1.0 / temperature)
    with np.errstate(over="ignore", invalid="ignore"):
        rep = (np.exp((vals * inv_t - gmax).astype(np.float32), dtype=np.float32) / denom).astype(np.float32)
    probs = rep.copy()
    if 0.0 < top_p < 1.0:
        total = np.float32(0)
        for p in probs:
            total = np.float32(total + p)
        cutoff, cum = np.float32(top_p) * total, np.float32(0)
        for j in range(k):
            if cum >= cutoff:
                probs[j] = 0.0
            else:
                cum = np.float32(cum + probs[j])
    if 0.0 < min_p < 1.0 and k:
        probs[np.float32(probs[0] * np.float32(min_p)) >= probs] = 0.0
    return ids, rep, probs


def sample(packed: np.ndarray, k: int, temperature: float, top_p: float, min_p: float, rng: np.random.Generator):
    """One draw: (token id, its reporting probability).  Raises like the reference when every weight is zero."""
    ids, rep, probs = filtered_probs(packed, k, temperature, top_p, min_p)
    # WeightedIndex::new (sampler.rs:1238-1258) refuses NaN / infinite / negative weights and an all-zero set; nothing is silently zeroed
    if float(np.where(np.isfinite(probs) & (probs > 0), probs, 0).astype(np.float64).sum()) == 0.0:
        raise ValueError("All sampling probabilities are zero after CUDA top-k filtering.")
    if not np.all(np.isfinite(probs)) or np.any(probs < 0):
        raise ValueError("Failed to construct CUDA top-k multinomial sampler: invalid weight")
    w = probs.astype(np.float64)
    j = int(rng.choice(k, p=w / w.sum()))
    return int(ids[j]), float(rep[j])


class Categorical:
    """Workspace + launcher of the device categorical draw over rows of `vocab` f32 logits (cuda_categorical_logits_f32_packed_batched, ops.rs:1347-1500)."""

    def __init__(self, vocab: int, device, max_rows: int = 1):
        vocab, max_rows = int(vocab), int(max_rows)
        if vocab <= 0:
            raise ValueError("categorical: empty logits")
        if vocab > 2 ** 24:
            raise ValueError(f"categorical: vocab={vocab} exceeds 2**24 (token ids come back as f32)")  # ops.rs:1387
        if max_rows < 1 or max_rows > 65535:
            raise ValueError(f"categorical: max_rows={max_rows} must be in [1, 65535]")
        self.vocab, self.max_rows, self.device = vocab, max_rows, device
        self.nblocks = (vocab + CHUNK_SIZE - 1) // CHUNK_SIZE
        f32 = dict(dtype=torch.float32, device=device)
        self.block_values = torch.empty(max_rows, self.nblocks, **f32)
        self.block_sums = torch.empty(max_rows, self.nblocks, **f32)
        self.packed = torch.empty(max_rows, 2, **f32)
        self._params = torch.empty(2, max_rows, **f32)  # [0] inverse temperatures, [1] uniforms: one upload
        vp, i, ll = C.c_void_p, C.c_int, C.c_int64
        self._many = _lib.sym("core", "categorical_large_f32_packed_batched", [vp, vp, vp, vp, vp, vp, i, i, i, i, ll])

    def __call__(self, logits: torch.Tensor, temperature, uniforms) -> torch.Tensor:
        """logits f32 [vocab] or [rows, vocab] (contiguous, on the device); temperature: a positive finite float, or one per row; uniforms: one value in [0, 1)
        per row.  Returns the packed rows [rows, 2] = (token id, logprob) on the device (a view of this object's buffer: consume it before the next call)."""
        x = logits.reshape(-1, self.vocab) if logits.dim() > 1 else logits.reshape(1, self.vocab)
        rows = x.shape[0]
        if x.dtype != torch.float32 or not x.is_contiguous() or rows > self.max_rows:
            raise ValueError("categorical: logits must be contiguous f32 with at most max_rows rows")
        temps = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (rows,))
        if not np.all(np.isfinite(temps) & (temps > 0)):
            raise ValueError("categorical requires a positive finite temperature")
        u = np.asarray(uniforms, dtype=np.float32).reshape(-1)
        if u.shape[0] != rows or not np.all((u >= 0) & (u < 1)):
            raise ValueError("categorical requires one uniform in [0, 1) per row")
        params = np.stack([(1.0 / temps).astype(np.float32), u])
        self._params[:, :rows].copy_(torch.from_numpy(params), non_blocking=False)
        self._many(x.data_ptr(), self._params[0].data_ptr(), self._params[1].data_ptr(), self.block_values.data_ptr(), self.block_sums.data_ptr(),
                   self.packed.data_ptr(), rows, self.vocab, CHUNK_SIZE, self.nblocks, torch.cuda.current_stream().cuda_stream)
        return self.packed[:rows]


def categorical_token(packed2):
    """Sampler::sample_cuda_categorical_row (sampler.rs:744-764): (token, logprob) of one packed pair; the token must be a finite non-negative integer, the logprob finite"""
    tok, lp = float(packed2[0]), float(packed2[1])
    if not (np.isfinite(tok) and np.isfinite(lp)) or tok < 0 or tok != np.floor(tok):
        raise ValueError("invalid batched CUDA categorical output")
    return int(tok), lp


def uniform_for(seed: int, index: int) -> np.float32:
    """The uniform in [0, 1) that draws token `index` of a request with `seed`: a function of (seed, index) alone, never of the call order -- a preempted and
    recomputed sequence redraws the same tokens.  The reference's distribution, not its Isaac64 stream."""
    return np.float32(np.random.default_rng((int(seed), int(index))).random(dtype=np.float32))


def categorical_host(logits_row, inv_temperature, uniform):
    """The contract of `categorical_large_f32_packed_batched` for one row in numpy f32 (one chunk, additions in index order): (token, logprob).  Raises like
    `categorical_token` where the device reports (NaN, NaN)."""
    x, inv_t, u = np.asarray(logits_row, dtype=np.float32).reshape(-1), np.float32(inv_temperature), np.float32(uniform)
    with np.errstate(over="ignore", invalid="ignore"):
        gmax = np.float32(x.max() * inv_t) if x.size else np.float32(np.nan)
        ok = np.isfinite(inv_t) and inv_t > 0 and np.isfinite(u) and 0 <= u < 1 and np.isfinite(gmax)
        if ok:
            w = np.exp((x * inv_t - gmax).astype(np.float32), dtype=np.float32)
            cum = np.cumsum(w, dtype=np.float32)  # sequential f32 additions
            denom = cum[-1]
            ok = np.isfinite(denom) and denom > 0
    if not ok:
        raise ValueError("invalid batched CUDA categorical output")
    target = min(np.float32(u * denom), np.nextafter(denom, np.float32(-np.inf)))
    hit = np.nonzero((w > 0) & (cum > target))[0]
    tok = int(hit[0]) if hit.size else int(np.nonzero(w > 0)[0][-1])
    return tok, float(np.float32(np.float32(x[tok] * inv_t - gmax) - np.log(denom, dtype=np.float32)))


class Nucleus:
    """Workspace + launcher of the device top-p / min-p draw over rows of `vocab` f32 logits (`mrs_nucleus_large_f32_packed_batched`; the reference has no device path
    for this case, sampler.rs:649-655).  Per-row temperature, uniform, top_p and min_p; a cut outside (0, 1) is inactive."""

    def __init__(self, vocab: int, device, max_rows: int = 1):
        vocab, max_rows = int(vocab), int(max_rows)
        if vocab <= 0:
            raise ValueError("nucleus: empty logits")
        if vocab > 2 ** 24:
            raise ValueError(f"nucleus: vocab={vocab} exceeds 2**24 (token ids come back as f32)")
        if max_rows < 1 or max_rows > 65535:
            raise ValueError(f"nucleus: max_rows={max_rows} must be in [1, 65535]")
        self.vocab, self.max_rows, self.device = vocab, max_rows, device
        self.nblocks = (vocab + CHUNK_SIZE - 1) // CHUNK_SIZE
        f32 = dict(dtype=torch.float32, device=device)
        self.block_values = torch.empty(max_rows, self.nblocks, **f32)
        self.block_sums = torch.empty(max_rows, self.nblocks, **f32)
        self.packed = torch.empty(max_rows, 4, **f32)
        self._params = torch.empty(4, max_rows, **f32)  # inverse temperatures, uniforms, top_p, min_p: one upload
        vp, i, ll = C.c_void_p, C.c_int, C.c_int64
        self._many = _lib.sym("core", "mrs_nucleus_large_f32_packed_batched", [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, ll])

    def __call__(self, logits: torch.Tensor, temperature, uniforms, top_p=1.0, min_p=0.0) -> torch.Tensor:
        """logits f32 [vocab] or [rows, vocab] (contiguous, on the device); temperature: positive and finite; uniforms: one value in [0, 1) per row; top_p / min_p: a
        float or one per row.  Returns the packed rows [rows, 4] = (token id, logprob under the full softmax, threshold logit x*, kept share of the mass) on the
        device (a view of this object's buffer: consume it before the next call)."""
        x = logits.reshape(-1, self.vocab) if logits.dim() > 1 else logits.reshape(1, self.vocab)
        rows = x.shape[0]
        if x.dtype != torch.float32 or not x.is_contiguous() or rows > self.max_rows:
            raise ValueError("nucleus: logits must be contiguous f32 with at most max_rows rows")
        temps = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (rows,))
        if not np.all(np.isfinite(temps) & (temps > 0)):
            raise ValueError("nucleus requires a positive finite temperature")
        u = np.asarray(uniforms, dtype=np.float32).reshape(-1)
        if u.shape[0] != rows or not np.all((u >= 0) & (u < 1)):
            raise ValueError("nucleus requires one uniform in [0, 1) per row")
        tp = np.broadcast_to(np.asarray(top_p, dtype=np.float32), (rows,))
        mp = np.broadcast_to(np.asarray(min_p, dtype=np.float32), (rows,))
        params = np.stack([(1.0 / temps).astype(np.float32), u, tp, mp])
        self._params[:, :rows].copy_(torch.from_numpy(params), non_blocking=False)
        pr = [self._params[j].data_ptr() for j in range(4)]
        self._many(x.data_ptr(), pr[0], pr[1], pr[2], pr[3], self.block_values.data_ptr(), self.block_sums.data_ptr(), self.packed.data_ptr(), rows, self.vocab,
                   CHUNK_SIZE, self.nblocks, torch.cuda.current_stream().cuda_stream)
        return self.packed[:rows]


def nucleus_token(packed4):
    """(token, logprob) of one packed row of the nucleus draw; raises on an unusable row (four NaNs), like `categorical_token`"""
    tok, lp = float(packed4[0]), float(packed4[1])
    if not (np.isfinite(tok) and np.isfinite(lp)) or tok < 0 or tok != np.floor(tok) or np.isnan(packed4[2]) or np.isnan(packed4[3]):
        raise ValueError("invalid batched nucleus output")
    return int(tok), lp


def cut_active(v) -> bool:
    """a top_p / min_p value cuts iff it lies strictly inside (0, 1) (sampler.rs:1625, 1645); None, NaN and everything else: no cut"""
    return v is not None and 0.0 < float(v) < 1.0


NUCLEUS_SCALE = 2.0 ** 39  # the fixed-point unit of csrc/sampling.hip: masses are integers, so their sums do not depend on the order of addition


def nucleus_host(logits_row, inv_temperature, uniform, top_p=1.0, min_p=0.0):
    """The contract of `mrs_nucleus_large_f32_packed_batched` for one row in numpy: (token, logprob, x*, kept share).  f32 weights, integer masses
    q_i = floor(w_i * 2^39); top-p keeps every logit >= x*, the largest logit at which the mass of the strictly greater logits is still below top_p * sum q (ALL ties
    at x* are kept); min-p keeps w_i > min_p; the draw inverts the cumulative kept mass in token order at min(floor(u * K), K - 1).  Raises where the device reports NaNs."""
    x, inv_t, u = np.asarray(logits_row, dtype=np.float32).reshape(-1), np.float32(inv_temperature), np.float32(uniform)
    tp, mp = np.float32(top_p), np.float32(min_p)
    with np.errstate(over="ignore", invalid="ignore"):
        gmax = np.float32(x.max() * inv_t) if x.size else np.float32(np.nan)
        ok = np.isfinite(inv_t) and inv_t > 0 and np.isfinite(u) and 0 <= u < 1 and np.isfinite(gmax)
        if ok:
            w = np.exp((x * inv_t - gmax).astype(np.float32), dtype=np.float32)
            denom = w.sum(dtype=np.float32)  # numpy's pairwise f32 sum: as close to the exact sum as the device's chunked trees
            ok = np.isfinite(denom) and denom > 0
    if not ok:
        raise ValueError("invalid batched nucleus output")
    q = (w.astype(np.float64) * NUCLEUS_SCALE).astype(np.uint64)  # exact: a power-of-two scale, then truncation
    total = int(q.sum(dtype=np.uint64))
    keep = np.ones(x.size, dtype=bool)
    xstar = np.float32(-np.inf)
    if 0.0 < tp < 1.0:
        order = np.argsort(-x, kind="stable")
        xs, qs = x[order], q[order]
        firsts = np.nonzero(np.r_[True, xs[1:] != xs[:-1]])[0]  # the first position of each distinct logit, descending
        above = np.r_[np.uint64(0), np.cumsum(qs, dtype=np.uint64)][firsts]  # the mass strictly above it
        cut = np.float64(tp) * np.float64(total)
        at = np.add.reduceat(qs, firsts)
        hit = np.nonzero((at > 0) & ((above + at).astype(np.float64) >= cut))[0][0]
        xstar = xs[firsts[hit]]
        keep &= x >= xstar
    if 0.0 < mp < 1.0:
        keep &= w > mp
    cum = np.cumsum(np.where(keep, q, np.uint64(0)), dtype=np.uint64)
    kept = int(cum[-1])
    target = min(int(np.float64(u) * np.float64(kept)), kept - 1)
    tok = int(np.searchsorted(cum, np.uint64(target), side="right"))
    lp = float(np.float32(np.float32(x[tok] * inv_t - gmax) - np.log(denom, dtype=np.float32)))
    return tok, lp, float(xstar), float(np.float32(np.float64(kept) / np.float64(total)))


def generate(model, prompt, max_new_tokens: int, top_k: int, temperature: float = 1.0, top_p: float = 1.0, min_p: float = 0.0, seed: int = 0,
             full_vocab_cuts: bool = False):
    """Sampled decoding on a `Llama` runner (the loop of `Sampler::sample`, sampler.rs:1262-1290): prefill, then per token one decode step and
      top_k >= 2: the device top-k over the logits row, `2k + 2` floats to the host, the top-p / min-p cuts and the draw there;
      top_k == 1: the arg-max through the top-1 kernels, no temperature, probability 1 (sample_cuda_top1_row);
      top_k <= 0 or None (top_p and min_p inactive): the device categorical draw over the whole row at `uniform_for(seed, i)` -- one launch pair, 2 floats to the host,
                 probability exp(logprob).  With an active top_p or min_p: `full_vocab_cuts=True` draws through `Nucleus` (the cuts over the WHOLE vocabulary on the
                 device, 4 floats to the host); without the keyword this raises, as the reference leaves the device there.
    Returns (tokens, reporting probabilities)."""
    vocab = int(model.cfg.vocab_size)
    if top_k is None or int(top_k) <= 0:
        cuts = 0.0 < top_p < 1.0 or 0.0 < min_p < 1.0
        if cuts and not full_vocab_cuts:
            raise ValueError("sampling with top_p / min_p needs top_k >= 1 (the device categorical draw takes the whole row)")
        k, t1, tk = 0, None, None
        cat = None if cuts else Categorical(vocab, model.device)
        nuc = Nucleus(vocab, model.device) if cuts else None
    else:
        k = min(int(top_k), vocab)
        t1 = Top1(vocab, model.device) if k == 1 else None
        tk = None if k == 1 else TopK(vocab, top_k, model.device)
    rng = np.random.default_rng(seed)
    logits = model.prefill(list(prompt), 0).float().reshape(1, -1)  # sequence 0: the decode steps below run batch row 0
    toks, probs = [], []
    for i in range(max_new_tokens):
        if hasattr(model, "p2p_sync_error") and model.p2p_sync_error():  # tensor parallel: a timed-out peer-mailbox sum is NaN -- never hand out a token from it
            raise RuntimeError("p2p all-reduce timed out: the route has been dropped on every rank (RCCL from now on); re-run the request")
        if k == 0 and nuc is not None:
            tok, lp = nucleus_token(nuc(logits.contiguous(), temperature, [uniform_for(seed, i)], top_p, min_p).cpu().numpy()[0])
            p = min(1.0, float(np.exp(lp)))
        elif k == 0:
            tok, lp = categorical_token(cat(logits.contiguous(), temperature, [uniform_for(seed, i)]).cpu().numpy()[0])
            p = min(1.0, float(np.exp(lp)))
        elif k == 1:  # sample_cuda_top1_row (sampler.rs:767-781): the arg-max, no temperature, logprob 0 (probability 1)
            tok, p = top1_token(t1(logits.contiguous()).cpu().numpy()[0]), 1.0
        else:
            packed = tk(logits.contiguous(), temperature).cpu().numpy()[0]
            tok, p = sample(packed, tk.k, temperature, top_p, min_p, rng)
        toks.append(tok)
        probs.append(p)
        if i + 1 < max_new_tokens:
            model.set_state([tok], [len(prompt) + i])
            logits = model.forward_logits(1)[0:1].float()
    return toks, probs
