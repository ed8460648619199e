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


class _Workspace:
    """What the four launchers below share: the shape checks and `nblocks`, the logits rows, and the per-row parameters.  `NAME` prefixes a class's refusals
    ("top-k: ..."); `NOUN` opens the ones about its parameters ("top-k requires ...").  The draws return token ids as f32 and put the rows into a grid dimension:
    `draw_limits` refuses what does not fit there (top-k and top-1 have no such limits)."""
    NAME = NOUN = ""

    def __init__(self, vocab, device, max_rows, draw_limits=False):
        if vocab <= 0:
            raise ValueError(f"{self.NAME}: empty logits")
        if draw_limits and vocab > 2 ** 24:
            raise ValueError(f"{self.NAME}: vocab={vocab} exceeds 2**24 (token ids come back as f32)")  # ops.rs:1387
        if draw_limits and (max_rows < 1 or max_rows > 65535):
            raise ValueError(f"{self.NAME}: max_rows={max_rows} must be in [1, 65535]")
        self.vocab, self.max_rows, self.device = vocab, max_rows, device
        self.nblocks = (vocab + CHUNK_SIZE - 1) // CHUNK_SIZE

    def _f32(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def _rows(self, logits):
        """the logits as [rows, vocab]: contiguous f32, at most max_rows rows"""
        x = logits.reshape(-1, self.vocab) if logits.dim() > 1 else logits.reshape(1, self.vocab)
        if x.dtype != torch.float32 or not x.is_contiguous() or x.shape[0] > self.max_rows:
            raise ValueError(f"{self.NAME}: logits must be contiguous f32 with at most max_rows rows")
        return x, x.shape[0]

    def _inv_temperatures(self, temperature, rows):
        """one positive finite temperature per row (or one for all) -> the f32 inverse temperatures"""
        temps = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (rows,))
        if not np.all(np.isfinite(temps) & (temps > 0)):
            raise ValueError(f"{self.NOUN} requires a positive finite temperature")
        return (1.0 / temps).astype(np.float32)

    def _uniforms(self, uniforms, rows):
        u = np.asarray(uniforms, dtype=np.float32).reshape(-1)
        if u.shape[0] != rows or not np.all((u >= 0) & (u < 1)):
            raise ValueError(f"{self.NOUN} requires one uniform in [0, 1) per row")
        return u

    def _upload(self, params, rows):
        """the stacked per-row parameters in ONE copy into self._params [len(params), max_rows]; returns the device pointer of each"""
        self._params[:, :rows].copy_(torch.from_numpy(np.stack(params)), non_blocking=False)
        return [self._params[j].data_ptr() for j in range(len(params))]


class TopK(_Workspace):
    """Workspace + launcher for rows of `vocab` f32 logits (cuda_topk_logits_f32_packed / _batched, ops.rs:691-1000)."""
    NAME = NOUN = "top-k"

    def __init__(self, vocab: int, k: int, device, max_rows: int = 1):
        k = min(int(k), int(vocab))
        super().__init__(vocab, device, max_rows)
        if k == 0 or k > MAX_K:
            raise ValueError(f"top-k: k={k} must be in [1, {MAX_K}]")
        self.k = k
        if self.nblocks * k > MAX_STAGE2:
            raise ValueError(f"top-k workspace too large: {self.nblocks * k} candidates")
        self.block_values = self._f32(max_rows, self.nblocks, k)
        self.block_indices = torch.empty(max_rows, self.nblocks, k, dtype=torch.int32, device=device)
        self.block_maxes, self.block_sums = self._f32(max_rows, self.nblocks), self._f32(max_rows, self.nblocks)
        self.packed = self._f32(max_rows, 2 * k + 2)
        self._params = self._f32(1, max_rows)  # the inverse temperatures of a batched call
        vp, i, f, ll = C.c_void_p, C.c_int, C.c_float, C.c_int64
        self._one = _lib.sym("core", "topk_large_f32_packed", [vp, vp, vp, vp, vp, vp, i, i, i, i, f, ll])
        self._many = _lib.sym("core", "topk_large_f32_packed_batched", [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, ll])

    def __call__(self, logits: torch.Tensor, temperature) -> torch.Tensor:
        """logits f32 [vocab] or [rows, vocab] (contiguous, on the device); temperature: a positive finite float, or one per row.  Returns the packed rows
        [rows, 2k + 2] on the device (a view of this object's buffer: consume it before the next call)."""
        x, rows = self._rows(logits)
        inv_t = self._inv_temperatures(temperature, rows)
        st = torch.cuda.current_stream().cuda_stream
        if rows == 1:
            self._one(x.data_ptr(), self.block_values.data_ptr(), self.block_indices.data_ptr(), self.block_maxes.data_ptr(), self.block_sums.data_ptr(),
                      self.packed.data_ptr(), self.vocab, self.k, CHUNK_SIZE, self.nblocks, float(inv_t[0]), st)
        else:
            self._many(x.data_ptr(), self._upload([inv_t], rows)[0], self.block_values.data_ptr(), self.block_indices.data_ptr(), self.block_maxes.data_ptr(),
                       self.block_sums.data_ptr(), self.packed.data_ptr(), rows, self.vocab, self.k, CHUNK_SIZE, self.nblocks, st)
        return self.packed[:rows]


class Top1(_Workspace):
    """Greedy rows: `top1_large_f32_packed[_batched]` (cuda_top1_logits_f32_*, ops.rs:1232-2050) -- packed [rows][2] = (max logit, token id as f32); no temperature."""
    NAME = "top-1"

    def __init__(self, vocab: int, device, max_rows: int = 1):
        super().__init__(vocab, device, max_rows)
        self.block_values = self._f32(max_rows, self.nblocks)
        self.block_indices = torch.empty(max_rows, self.nblocks, dtype=torch.int32, device=device)
        self.packed = self._f32(max_rows, 2)
        vp, i, ll = C.c_void_p, C.c_int, C.c_int64
        self._many = _lib.sym("core", "top1_large_f32_packed_batched", [vp, vp, vp, vp, vp, i, i, i, i, ll])

    def __call__(self, logits: torch.Tensor) -> torch.Tensor:
        x, rows = self._rows(logits.reshape(-1, self.vocab))
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


class Categorical(_Workspace):
    """Workspace + launcher of the device categorical draw over rows of `vocab` f32 logits (cuda_categorical_logits_f32_packed_batched, ops.rs:1347-1500)."""
    NAME = NOUN = "categorical"

    def __init__(self, vocab: int, device, max_rows: int = 1):
        super().__init__(int(vocab), device, int(max_rows), draw_limits=True)
        self.block_values, self.block_sums = self._f32(self.max_rows, self.nblocks), self._f32(self.max_rows, self.nblocks)
        self.packed = self._f32(self.max_rows, 2)
        self._params = self._f32(2, self.max_rows)  # [0] inverse temperatures, [1] uniforms: one upload
        vp, i, ll = C.c_void_p, C.c_int, C.c_int64
        self._many = _lib.sym("core", "categorical_large_f32_packed_batched", [vp, vp, vp, vp, vp, vp, i, i, i, i, ll])

    def __call__(self, logits: torch.Tensor, temperature, uniforms) -> torch.Tensor:
        """logits f32 [vocab] or [rows, vocab] (contiguous, on the device); temperature: a positive finite float, or one per row; uniforms: one value in [0, 1)
        per row.  Returns the packed rows [rows, 2] = (token id, logprob) on the device (a view of this object's buffer: consume it before the next call)."""
        x, rows = self._rows(logits)
        pr = self._upload([self._inv_temperatures(temperature, rows), self._uniforms(uniforms, rows)], rows)
        self._many(x.data_ptr(), pr[0], pr[1], self.block_values.data_ptr(), self.block_sums.data_ptr(),
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


def _host_weights(logits_row, inv_temperature, uniform):
    """The opening of both host rules: (x, inv_t, u, gmax, w) with the f32 weights w = exp(x * inv_t - gmax) -- all of them in [0, 1] -- or w = None where inv_t, u or
    gmax already make the row unusable.  The rules add the weights into `denom` each in its own way, ON PURPOSE."""
    x, inv_t, u = np.asarray(logits_row, dtype=np.float32).reshape(-1), np.float32(inv_temperature), np.float32(uniform)
    with np.errstate(over="ignore", invalid="ignore"):
        gmax = np.float32(x.max() * inv_t) if x.size else np.float32(np.nan)
        ok = np.isfinite(inv_t) and inv_t > 0 and np.isfinite(u) and 0 <= u < 1 and np.isfinite(gmax)
        w = np.exp((x * inv_t - gmax).astype(np.float32), dtype=np.float32) if ok else None
    return x, inv_t, u, gmax, w


def categorical_host(logits_row, inv_temperature, uniform):
    """The contract of `categorical_large_f32_packed_batched` for one row in numpy f32 (one chunk, additions in index order): (token, logprob).  Raises like
    `categorical_token` where the device reports (NaN, NaN)."""
    x, inv_t, u, gmax, w = _host_weights(logits_row, inv_temperature, uniform)
    if w is not None:
        cum = np.cumsum(w, dtype=np.float32)  # SEQUENTIAL f32 additions: the running sums the draw inverts, denom their last (nucleus_host: a pairwise sum)
        denom = cum[-1]
    if w is None or not (np.isfinite(denom) and denom > 0):
        raise ValueError("invalid batched CUDA categorical output")
    target = min(np.float32(u * denom), np.nextafter(denom, np.float32(-np.inf)))
    hit = np.nonzero((w > 0) & (cum > target))[0]
    tok = int(hit[0]) if hit.size else int(np.nonzero(w > 0)[0][-1])
    return tok, float(np.float32(np.float32(x[tok] * inv_t - gmax) - np.log(denom, dtype=np.float32)))


class Nucleus(_Workspace):
    """Workspace + launcher of the device top-p / min-p draw over rows of `vocab` f32 logits (`mrs_nucleus_large_f32_packed_batched`; the reference has no device path
    for this case, sampler.rs:649-655).  Per-row temperature, uniform, top_p and min_p; a cut outside (0, 1) is inactive."""
    NAME = NOUN = "nucleus"

    def __init__(self, vocab: int, device, max_rows: int = 1):
        super().__init__(int(vocab), device, int(max_rows), draw_limits=True)
        self.block_values, self.block_sums = self._f32(self.max_rows, self.nblocks), self._f32(self.max_rows, self.nblocks)
        self.packed = self._f32(self.max_rows, 4)
        self._params = self._f32(4, self.max_rows)  # inverse temperatures, uniforms, top_p, min_p: one upload
        vp, i, ll = C.c_void_p, C.c_int, C.c_int64
        self._many = _lib.sym("core", "mrs_nucleus_large_f32_packed_batched", [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, ll])

    def __call__(self, logits: torch.Tensor, temperature, uniforms, top_p=1.0, min_p=0.0) -> torch.Tensor:
        """logits f32 [vocab] or [rows, vocab] (contiguous, on the device); temperature: positive and finite; uniforms: one value in [0, 1) per row; top_p / min_p: a
        float or one per row.  Returns the packed rows [rows, 4] = (token id, logprob under the full softmax, threshold logit x*, kept share of the mass) on the
        device (a view of this object's buffer: consume it before the next call)."""
        x, rows = self._rows(logits)
        cuts = [np.broadcast_to(np.asarray(c, dtype=np.float32), (rows,)) for c in (top_p, min_p)]
        pr = self._upload([self._inv_temperatures(temperature, rows), self._uniforms(uniforms, rows), *cuts], rows)
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
    x, inv_t, u, gmax, w = _host_weights(logits_row, inv_temperature, uniform)
    if w is not None:
        denom = w.sum(dtype=np.float32)  # numpy's PAIRWISE f32 sum: as close to the exact sum as the device's chunked trees (categorical_host: sequential)
    if w is None or not (np.isfinite(denom) and denom > 0):
        raise ValueError("invalid batched nucleus output")
    tp, mp = np.float32(top_p), np.float32(min_p)
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


MAX_BIAS = 1024  # logit-bias entries per row that a `Penalties` workspace has room for


def _f32_or(v, default):
    with np.errstate(over="ignore"):
        return np.float32(default if v is None else v)


def _token_ids(tokens, what):
    """token ids as uint32; refuses negative, non-integer and > 32-bit ids"""
    try:
        a = np.asarray(list(tokens) if not isinstance(tokens, np.ndarray) else tokens)
        a = a.reshape(-1) if a.size else np.zeros(0, np.int64)
        ok = a.dtype.kind in "iuf" and bool(np.all(np.isfinite(a) & (a >= 0) & (a < 2 ** 32) & (a == np.floor(a))))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"penalties: {what} must be non-negative integer token ids")
    return a.astype(np.uint32)


def check_penalties(frequency_penalty=None, presence_penalty=None, repetition_penalty=None, logit_bias=None):
    """The refusals that `Penalties`, `penalties_host` and the engine share (None: the inactive default).  Returns the f32 triple and the bias as (ids uint32, values f32)
    with the zero entries dropped (sampler.rs:1153-1158 drops them too)."""
    f, p, rp = _f32_or(frequency_penalty, 0.0), _f32_or(presence_penalty, 0.0), _f32_or(repetition_penalty, 1.0)
    if not (np.isfinite(f) and np.isfinite(p) and np.isfinite(rp)):
        raise ValueError("penalties: frequency, presence and repetition penalty must be finite")
    if rp <= 0:
        raise ValueError("penalties: repetition_penalty must be > 0")
    if logit_bias is None:
        logit_bias = {}
    if not isinstance(logit_bias, dict):
        raise ValueError("penalties requires logit_bias as a dict {token id: bias}")
    ids = _token_ids(list(logit_bias.keys()), "logit_bias keys")
    try:
        with np.errstate(over="ignore"):
            vals = np.asarray(list(logit_bias.values()), dtype=np.float64).astype(np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("penalties: logit_bias values must be finite numbers") from None
    if not np.all(np.isfinite(vals)):
        raise ValueError("penalties: logit_bias values must be finite numbers")
    if np.unique(ids).size != ids.size:
        raise ValueError("penalties requires unique logit_bias token ids")
    keep = vals != 0
    if int(keep.sum()) > MAX_BIAS:
        raise ValueError(f"penalties requires at most {MAX_BIAS} logit_bias entries per row")
    return f, p, rp, ids[keep], vals[keep]


def penalties_active(frequency_penalty, presence_penalty, repetition_penalty, logit_bias) -> bool:
    """True iff the setting changes a row: f != 0, p != 0, rp != 1 or a non-zero bias entry; None is inactive (a NaN is active, and refused by check_penalties)"""
    f, p, rp = frequency_penalty, presence_penalty, repetition_penalty
    if (f is not None and float(f) != 0.0) or (p is not None and float(p) != 0.0) or (rp is not None and float(rp) != 1.0):
        return True
    return bool(logit_bias) and any(float(v) != 0.0 for v in logit_bias.values())


class Penalties(_Workspace):
    """Workspace + launcher of the batched pre-processing of rows of `vocab` f32 logits (`mrs_penalties_f32_batched`; the reference has no batched device plan for a request
    with penalties, sampler.rs:617-631): frequency / presence penalties over the GENERATED tokens, the repetition penalty over the WHOLE context, then the additive bias
    -- sampler.rs:1090-1169.  The raw token history goes up; the device counts.  One call = two uploads (int32 and f32 parameters) + one launch."""
    NAME = NOUN = "penalties"

    def __init__(self, vocab: int, device, max_rows: int = 1, max_context: int = 1 << 16):
        super().__init__(int(vocab), device, int(max_rows))
        if self.max_rows < 1 or self.max_rows > 65535:  # the rows are a grid dimension
            raise ValueError(f"penalties: max_rows={max_rows} must be in [1, 65535]")
        if int(max_context) < 0:
            raise ValueError(f"penalties: max_context={max_context} must not be negative")
        self.max_context = int(max_context)
        self.dst = self._f32(self.max_rows, self.vocab)
        # int32: context offsets [rows + 1], prompt lengths [rows], bias offsets [rows + 1], bias ids, context tokens; f32: the three penalties [rows] each, bias values
        self._ints = torch.empty(3 * self.max_rows + 2 + self.max_rows * MAX_BIAS + self.max_context, dtype=torch.int32, device=device)
        self._floats = self._f32(3 * self.max_rows + self.max_rows * MAX_BIAS)
        vp, i, ll = C.c_void_p, C.c_int, C.c_int64
        self._many = _lib.sym("core", "mrs_penalties_f32_batched", [vp] * 11 + [i, i, i, ll])

    def _per_row(self, v, default, rows):
        try:
            return np.broadcast_to(np.asarray(default if v is None else v, dtype=np.float64), (rows,))
        except (TypeError, ValueError):
            raise ValueError("penalties requires one penalty value per row, or one for all") from None

    def __call__(self, logits: torch.Tensor, contexts, prompt_lens, frequency_penalty=0.0, presence_penalty=0.0, repetition_penalty=1.0, logit_bias=None) -> torch.Tensor:
        """logits f32 [vocab] or [rows, vocab] (contiguous, on the device); contexts: one token-id sequence per row (prompt + generated so far, may be empty);
        prompt_lens: how many leading tokens of each context are the prompt (an int, or one per row); the penalties: a float or one per row; logit_bias: a dict
        {token id: bias} for all rows, or a list with one dict (or None) per row -- entries equal to 0 or with an id >= vocab are dropped.  Returns the updated rows
        [rows, vocab] on the device (a view of this object's buffer: consume it before the next call); `logits` is left as it is."""
        x, rows = self._rows(logits)
        if not isinstance(contexts, (list, tuple)) or len(contexts) != rows or any(np.isscalar(c) for c in contexts):
            raise ValueError("penalties requires one context (a sequence of token ids) per row")
        ctx = [_token_ids(c, "context tokens") for c in contexts]
        try:
            pl = np.broadcast_to(np.asarray(prompt_lens), (rows,))
            ok = pl.dtype.kind in "iu" and bool(np.all(pl >= 0))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("penalties requires one non-negative integer prompt length per row, or one for all")
        biases = logit_bias if isinstance(logit_bias, (list, tuple)) else [logit_bias] * rows
        if len(biases) != rows:
            raise ValueError("penalties requires one logit_bias dict per row, or one for all")
        fs, ps, rps = (self._per_row(v, d, rows) for v, d in ((frequency_penalty, 0.0), (presence_penalty, 0.0), (repetition_penalty, 1.0)))
        par = [check_penalties(fs[r], ps[r], rps[r], biases[r]) for r in range(rows)]
        bias = [(ids[ids < self.vocab], vals[ids < self.vocab]) for _, _, _, ids, vals in par]
        offsets = np.concatenate([[0], np.cumsum([c.size for c in ctx])]).astype(np.int64)
        if offsets[-1] > self.max_context:
            raise ValueError(f"penalties: {int(offsets[-1])} context tokens exceed max_context={self.max_context}")
        boffsets = np.concatenate([[0], np.cumsum([b[0].size for b in bias])]).astype(np.int64)
        ints = np.concatenate([offsets, np.minimum(pl, 2 ** 31 - 1).astype(np.int64), boffsets, *[b[0] for b in bias], *ctx]).astype(np.uint32).view(np.int32)
        floats = np.concatenate([[q[j] for q in par] for j in range(3)] + [b[1] for b in bias]).astype(np.float32)
        self._ints[:ints.size].copy_(torch.from_numpy(ints), non_blocking=False)
        self._floats[:floats.size].copy_(torch.from_numpy(floats), non_blocking=False)
        ip, fp = self._ints.data_ptr(), self._floats.data_ptr()
        at = lambda base, n: base + 4 * n
        has_bias = boffsets[-1] > 0
        self._many(x.data_ptr(), self.dst.data_ptr(), at(ip, 3 * rows + 2 + int(boffsets[-1])), ip, at(ip, rows + 1), fp, at(fp, rows), at(fp, 2 * rows),
                   at(ip, 3 * rows + 2) if has_bias else None, at(fp, 3 * rows) if has_bias else None, at(ip, 2 * rows + 1) if has_bias else None,
                   rows, self.vocab, CHUNK_SIZE, torch.cuda.current_stream().cuda_stream)
        return self.dst[:rows]


def penalties_host(logits_row, context, prompt_len, frequency_penalty=0.0, presence_penalty=0.0, repetition_penalty=1.0, logit_bias=None):
    """The contract of `mrs_penalties_f32_batched` for one row in numpy f32: the updated row.  With g = occurrences of a token among context[prompt_len:] and s = its
    occurrences in the whole context: v = x; g > 0: v -= g * f + p; s > 0 and rp != 1: v = v > 0 ? v / rp : v * rp; then v += bias.  Token ids >= the row's length are
    ignored; bias entries equal to 0 are dropped.
    The device evaluates g * f + p as ONE fused multiply-add; here it is a float64 product and sum rounded once to f32.  The float64 sum is exact -- and this rule equal to
    the device BIT FOR BIT -- whenever the counts are <= 4096 and each penalty is 0 or has a magnitude in [2^-10, 8]: the product then has at most 13 + 24 - 1 = 36
    significant bits and the two terms together span fewer than 53."""
    x = np.array(logits_row, dtype=np.float32).reshape(-1)
    n = x.size
    f, p, rp, ids, vals = check_penalties(frequency_penalty, presence_penalty, repetition_penalty, logit_bias)
    ctx = _token_ids(context, "context tokens")
    if not isinstance(prompt_len, (int, np.integer)) or prompt_len < 0:
        raise ValueError("penalties requires one non-negative integer prompt length per row, or one for all")
    gen = ctx[min(int(prompt_len), ctx.size):]
    g = np.bincount(gen[gen < n], minlength=n)
    s = np.bincount(ctx[ctx < n], minlength=n)
    with np.errstate(over="ignore", invalid="ignore"):
        hit = g > 0
        x[hit] = x[hit] - (g[hit].astype(np.float64) * np.float64(f) + np.float64(p)).astype(np.float32)
        if rp != np.float32(1.0):
            hit = s > 0
            v = x[hit]
            x[hit] = np.where(v > 0, v / rp, v * rp)
        ids, vals = ids[ids < n], vals[ids < n]
        x[ids] = x[ids] + vals
    return x


def generate(model, prompt, max_new_tokens: int, top_k: int, temperature: float = 1.0, top_p: float = 1.0, min_p: float = 0.0, seed: int = 0,
             full_vocab_cuts: bool = False, frequency_penalty: float = 0.0, presence_penalty: float = 0.0, repetition_penalty: float = 1.0, logit_bias=None):
    """Sampled decoding on a `Llama` runner (the loop of `Sampler::sample`, sampler.rs:1262-1290): prefill, then per token one decode step and
      top_k >= 2: the device top-k over the logits row, `2k + 2` floats to the host, the top-p / min-p cuts and the draw there;
      top_k == 1: the arg-max through the top-1 kernels, no temperature, probability 1 (sample_cuda_top1_row);
      top_k <= 0 or None (top_p and min_p inactive): the device categorical draw over the whole row at `uniform_for(seed, i)` -- one launch pair, 2 floats to the host,
                 probability exp(logprob).  With an active top_p or min_p: `full_vocab_cuts=True` draws through `Nucleus` (the cuts over the WHOLE vocabulary on the
                 device, 4 floats to the host); without the keyword this raises, as the reference leaves the device there.
    With an active penalty or logit bias (`penalties_active`) the row first goes through `Penalties` -- context = prompt + tokens so far, the prompt's tokens not
    "generated" -- and the updated row takes the place of the raw one in all three modes (the reference applies them before everything else, sampler.rs:1853).
    Returns (tokens, reporting probabilities)."""
    vocab = int(model.cfg.vocab_size)
    pen = None
    if penalties_active(frequency_penalty, presence_penalty, repetition_penalty, logit_bias):
        check_penalties(frequency_penalty, presence_penalty, repetition_penalty, logit_bias)
        pen = Penalties(vocab, model.device, max_context=len(prompt) + max_new_tokens)
    if top_k is None or int(top_k) <= 0:
        cuts = 0.0 < top_p < 1.0 or 0.0 < min_p < 1.0
        if cuts and not full_vocab_cuts:
            raise ValueError("sampling with top_p / min_p needs top_k >= 1 (the device categorical draw takes the whole row)")
        k, t1, tk = 0, None, None
        draw = Nucleus(vocab, model.device) if cuts else Categorical(vocab, model.device)
        parse, extra = (nucleus_token, (top_p, min_p)) if cuts else (categorical_token, ())
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
        if pen is not None:
            logits = pen(logits.contiguous(), [list(prompt) + toks], len(prompt), frequency_penalty, presence_penalty, repetition_penalty, logit_bias)
        if k == 0:  # one launch pair of the whole-row draw in use, (token, logprob) parsed from its packed row
            tok, lp = parse(draw(logits.contiguous(), temperature, [uniform_for(seed, i)], *extra).cpu().numpy()[0])
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
