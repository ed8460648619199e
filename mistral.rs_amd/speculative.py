"""Speculative decoding: the role of mistralrs-core/src/speculative/ (verifier.rs:44-115 greedy verification, :200-290 the accept loop, :339-473 the stochastic rule).

A proposer drafts k <= 7 tokens; ONE verify step of the target (`Llama.verify_step`: the anchor token and the drafts as rows of one sequence through the batched decode
launches) scores all of them; `mrs_spec_verify_f32_batched` (csrc/sampling.hip) judges the round on the device and `mrs_spec_advance` (csrc/ext_decode.hip) moves the
decode state past the accepted tokens.  The reference runs the accept loop on the host over full-vocabulary probability vectors; here the host reads back
(n_accepted, out_tokens) -- nine integers -- once per round.

The batched decode launches produce the bits of the batch-1 step, so GREEDY speculative decoding is lossless at the level of token ids and of logits bits,
whatever the proposer does.  At a temperature the emitted tokens follow the target's distribution (the law of the accept / residual rule), not the plain run's stream.

Uniforms are functions of (seed, token index) alone, on three disjoint streams of `sampler.uniform_for` -- with t the index of the generated token a row would emit:
    u1 (the draw if the row ends the round)   uniform_for(seed, t)            -- the stream of `sampler.generate(top_k=0)`: without drafts the two runs draw the same tokens
    u0 (the accept draw of the draft for t)   uniform_for(seed, 2**31 + t)
    the draft model's own draw of token t     uniform_for(seed, 2**32 + t)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, sampler
from .sampler import CHUNK_SIZE, _Workspace, uniform_for

MAX_ROWS = 8   # rows of one sequence in a round: the anchor + at most 7 drafts
GREEDY, TEMPERATURE = 0, 1
U0_STREAM, DRAFT_STREAM = 2 ** 31, 2 ** 32


class SpecVerify(_Workspace):
    """Workspace + launcher of `mrs_spec_verify_f32_batched` over rows of `vocab` f32 logits: up to `max_seqs` sequences of 1..8 rows each in one launch group."""
    NAME = NOUN = "speculative verify"

    def __init__(self, vocab: int, device, max_seqs: int = 1, max_rows: int | None = None):
        max_seqs = int(max_seqs)
        max_rows = MAX_ROWS * max_seqs if max_rows is None else int(max_rows)
        if max_seqs < 1 or max_rows < max_seqs or max_rows > MAX_ROWS * max_seqs:
            raise ValueError(f"speculative verify: max_seqs={max_seqs}, max_rows={max_rows}: every sequence has 1..{MAX_ROWS} rows")
        super().__init__(int(vocab), device, max_rows, draw_limits=True)
        self.max_seqs = max_seqs
        vp, i, ll, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
        need = int(_lib.sym("core", "mrs_spec_verify_workspace_bytes", [i, i, i], sz)(max_rows, max_seqs, self.nblocks))
        self.workspace = torch.empty(need + 8, dtype=torch.uint8, device=device)
        self.result = torch.full((max_seqs * (1 + MAX_ROWS),), -1, dtype=torch.int32, device=device)  # n_accepted [max_seqs], then out_tokens [max_seqs][8]: ONE read-back
        self.n_accepted, self.out_tokens = self.result[:max_seqs], self.result[max_seqs:].view(max_seqs, MAX_ROWS)
        self._ints = torch.empty(2 * max_seqs + 1 + max_rows, dtype=torch.int32, device=device)  # seq_rows [nseq + 1], modes [nseq], draft ids [rows]
        self._floats = self._f32(max_seqs + 2 * max_rows)                                         # inverse temperatures [nseq], uniforms [rows][2]
        self._launch = _lib.sym("core", "mrs_spec_verify_f32_batched", [vp] * 8 + [sz, vp, vp, i, i, i, i, i, ll])

    def __call__(self, target_logits: torch.Tensor, draft_ids, seq_rows, temperature=0.0, uniforms=None, draft_logits: torch.Tensor | None = None):
        """target_logits f32 [rows, vocab] (contiguous, on the device); draft_ids: one id per row (the bonus rows' entries are ignored) as a host sequence, or the
        device address of an int32 array; seq_rows: nseq + 1 ascending row offsets; temperature: 0 = greedy, > 0 = the stochastic rule -- one value or one per sequence;
        uniforms [rows, 2] in [0, 1) (needed by temperature sequences); draft_logits: the proposer's rows, same shape, or None for a deterministic proposer.
        Returns (n_accepted [nseq], out_tokens [nseq, 8]) on the device: views of `self.result` -- read that ONE tensor back, before the next call."""
        x, rows = self._rows(target_logits)
        sr = np.asarray(seq_rows, dtype=np.int64).reshape(-1)
        nseq = sr.size - 1
        if nseq < 1 or nseq > self.max_seqs or sr[0] != 0 or sr[-1] != rows or np.any(np.diff(sr) < 1) or np.any(np.diff(sr) > MAX_ROWS):
            raise ValueError(f"speculative verify requires seq_rows = nseq + 1 ascending offsets over the rows, 1..{MAX_ROWS} rows per sequence, at most {self.max_seqs} sequences")
        temps = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (nseq,))
        if not np.all(np.isfinite(temps) & (temps >= 0)):
            raise ValueError("speculative verify requires a finite temperature >= 0 (0 = greedy)")
        modes = np.where(temps > 0, TEMPERATURE, GREEDY).astype(np.int64)
        inv_t = (1.0 / np.where(temps > 0, temps, 1.0)).astype(np.float32)
        if uniforms is None:
            if modes.any():
                raise ValueError("speculative verify requires uniforms [rows, 2] for a temperature sequence")
            u = np.zeros(2 * rows, np.float32)
        else:
            u = np.asarray(uniforms, dtype=np.float32).reshape(-1)
            if u.size != 2 * rows or not np.all((u >= 0) & (u < 1)):
                raise ValueError("speculative verify requires two uniforms in [0, 1) per row")
        q = None
        if draft_logits is not None:
            q, qrows = self._rows(draft_logits)
            if qrows != rows:
                raise ValueError("speculative verify: draft_logits must have the target's shape")
        ints = [sr, modes]
        on_device = isinstance(draft_ids, (int, np.integer))
        if not on_device:
            ids = np.asarray(draft_ids, dtype=np.int64).reshape(-1)
            if ids.size != rows:
                raise ValueError("speculative verify requires one draft id per row (the bonus rows' entries are ignored)")
            ints.append(np.clip(ids, -1, 2 ** 31 - 1))
        ints = np.concatenate(ints).astype(np.int32)
        floats = np.concatenate([inv_t, u]).astype(np.float32)
        self._ints[:ints.size].copy_(torch.from_numpy(ints), non_blocking=False)
        self._floats[:floats.size].copy_(torch.from_numpy(floats), non_blocking=False)
        ip, fp = self._ints.data_ptr(), self._floats.data_ptr()
        ws = (self.workspace.data_ptr() + 7) & ~7
        self._launch(x.data_ptr(), q.data_ptr() if q is not None else None, int(draft_ids) if on_device else ip + 4 * (2 * nseq + 1), ip, ip + 4 * (nseq + 1), fp,
                     fp + 4 * nseq, ws, self.workspace.numel() - 8, self.n_accepted.data_ptr(), self.out_tokens.data_ptr(), nseq, rows, self.vocab, CHUNK_SIZE,
                     self.nblocks, torch.cuda.current_stream().cuda_stream)
        return self.n_accepted[:nseq], self.out_tokens[:nseq]


def _softmax_host(row, inv_t, u):
    """(x, w, cum, denom) of one row as `categorical_host` computes them, or raises where the device reports an unusable row"""
    x, inv_t, u, gmax, w = sampler._host_weights(row, inv_t, u)
    if w is not None:
        cum = np.cumsum(w, dtype=np.float32)
        denom = cum[-1]
    if w is None or not (np.isfinite(denom) and denom > 0):
        raise ValueError("invalid speculative verify row")
    return x, w, cum, denom


def verify_host(target_rows, draft_ids, temperature=0.0, uniforms=None, draft_rows=None):
    """The contract of `mrs_spec_verify_f32_batched` for ONE sequence in numpy f32 (one chunk, additions in index order): (n_accepted, tokens) with tokens = the accepted
    drafts + the continuation.  target_rows [n + 1, vocab]; draft_ids: n ids (further entries are ignored); temperature 0 = greedy; uniforms [n + 1, 2] = (u0, u1).
      greedy: a row's winner is its largest value, lowest index on ties, -0.0 ranking with +0.0; drafts are accepted while winner == draft; the continuation is the winner
      of the first other row.
      temperature: p = softmax(target / T), q = softmax(draft / T) -- one-hot on the draft without draft_rows; accept = q_d > 0 ? min(1, p_d / q_d) : (p_d > 0 ? 1 : 0);
      accepted iff u0 < accept.  The first rejected row draws from max(p - q, 0) by inverting its running sums at u1 (from p when they sum to nothing); with every draft
      accepted the bonus row is `categorical_host` at u1.  Rows after the one that ends the round are not looked at.  Raises ValueError where the device reports -1."""
    t = np.asarray(target_rows, dtype=np.float32)
    t = t.reshape(1, -1) if t.ndim == 1 else t
    n, vocab = t.shape[0] - 1, t.shape[1]
    ids = [int(d) for d in np.asarray(draft_ids).reshape(-1)[:n]]
    if len(ids) < n or n >= MAX_ROWS:
        raise ValueError("verify_host requires one draft id per judged row, at most 7")
    out = []
    if not temperature > 0:
        for i in range(n + 1):
            if np.isnan(t[i]).any():
                raise ValueError("invalid speculative verify row")
            winner = int(np.argmax(t[i] + np.float32(0.0)))
            if i < n and winner == ids[i]:
                out.append(winner)
                continue
            return len(out), out + [winner]
    inv_t = np.float32(1.0 / np.float64(temperature))
    us = np.asarray(uniforms, dtype=np.float32).reshape(n + 1, 2)
    q_rows = None if draft_rows is None else np.asarray(draft_rows, dtype=np.float32).reshape(-1, vocab)
    for i in range(n):
        d, u0, u1 = ids[i], us[i, 0], us[i, 1]
        _, wp, _, dp = _softmax_host(t[i], inv_t, u0)
        if not 0 <= d < vocab:
            raise ValueError("invalid speculative verify row")
        p = (wp / dp).astype(np.float32)
        if q_rows is None:
            qd, res = np.float32(1.0), p.copy()
            res[d] = 0.0
        else:
            _, wq, _, dq = _softmax_host(q_rows[i], inv_t, u0)
            q = (wq / dq).astype(np.float32)
            qd, res = q[d], np.maximum(p - q, np.float32(0.0)).astype(np.float32)
        accept = min(np.float32(1.0), np.float32(p[d] / qd)) if qd > 0 else np.float32(1.0 if p[d] > 0 else 0.0)
        if u0 < accept:
            out.append(d)
            continue
        cum = np.cumsum(res, dtype=np.float32)
        total = cum[-1]
        if total > 0 and np.isfinite(total):
            if not 0 <= u1 < 1:
                raise ValueError("invalid speculative verify row")
            target = min(np.float32(u1 * total), np.nextafter(total, np.float32(-np.inf)))
            hit = np.nonzero((res > 0) & (cum > target))[0]
            tok = int(hit[0]) if hit.size else int(np.nonzero(res > 0)[0][-1])
        else:
            try:
                tok = sampler.categorical_host(t[i], inv_t, u1)[0]
            except ValueError:
                raise ValueError("invalid speculative verify row") from None
        return len(out), out + [tok]
    try:
        tok = sampler.categorical_host(t[n], inv_t, us[n, 1])[0]
    except ValueError:
        raise ValueError("invalid speculative verify row") from None
    return n, out + [tok]


class NGramProposer:
    """Prompt lookup: the longest earlier match (at most `n` tokens long) of the context's last tokens; proposes the up to `k` tokens that followed its most recent
    occurrence.  Deterministic: no draft logits, q is one-hot on each draft."""

    def __init__(self, n: int = 3, k: int = 4):
        if n < 1 or k < 1 or k >= MAX_ROWS:
            raise ValueError(f"NGramProposer: n >= 1 and 1 <= k <= {MAX_ROWS - 1}")
        self.n, self.k = int(n), int(k)

    def reset(self):
        pass

    def propose(self, context, k_max: int, temperature: float = 0.0, seed: int = 0, n_generated: int = 0):
        ctx = list(context)
        k = min(self.k, int(k_max))
        for length in range(min(self.n, len(ctx) - 1), 0, -1):
            tail = ctx[-length:]
            for start in range(len(ctx) - length - 1, -1, -1):  # the most recent earlier occurrence first
                if ctx[start:start + length] == tail:
                    follow = ctx[start + length:start + length + k]
                    if follow:
                        return follow, None
        return [], None


class DraftModelProposer:
    """A second `Llama` with the target's vocabulary drafts with its own batch-1 decode steps, greedy or at the request's temperature, and hands over the logits row each
    draft was drawn from.  The draft of generated token t is drawn at uniform_for(seed, 2**32 + t): a function of (seed, token index) alone, disjoint from the verifier's
    streams (see the module docstring).  Before it drafts again it catches up on the accepted tokens it has not processed -- the tokens where its pages and the new context
    part -- in one multi-row step (`Llama.verify_step` on the draft model; a longer gap, the prompt, goes through its prompt path).  Inside `generate_speculative` that
    gap is at most ONE token (the last accepted draft: the proposer has processed every draft but the last); gaps of 2..8 arise when a proposer is handed a context it
    did not draft itself, and take the same step with more rows."""

    def __init__(self, llama, seq: int = 0):
        self.m, self.seq = llama, int(seq)
        vocab = int(llama.cfg.vocab_size)
        self.logits = torch.zeros(MAX_ROWS, vocab, dtype=torch.float32, device=llama.device)  # one row per draft + the bonus row's (never judged) place
        self._top1, self._cat = sampler.Top1(vocab, llama.device), sampler.Categorical(vocab, llama.device)
        self.reset()

    def reset(self):
        self.done = []  # the tokens whose K/V sit in the draft model's pages, position by position

    def _catch_up(self, ctx):
        """make the pages hold ctx[:-1]; ctx[-1] is the next anchor"""
        m, want = self.m, ctx[:-1]
        keep = 0
        while keep < min(len(self.done), len(want)) and self.done[keep] == want[keep]:
            keep += 1
        gap = want[keep:]
        rows = min(MAX_ROWS, int(m.cfg.max_batch))
        if len(gap) > rows and self.seq == 0:
            if m.prefill_is_exact or m.cfg.kv_dtype == "bf16":
                m.prefill(gap, keep, seq=0)
            else:
                m.prefill_chunked(gap, keep)
        else:
            for i in range(0, len(gap), rows):
                part = gap[i:i + rows]
                m.set_state_seq(self.seq, part[0], keep + i)
                m.verify_step(self.seq, len(part), part[1:])
        self.done = list(want)

    def propose(self, context, k_max: int, temperature: float = 0.0, seed: int = 0, n_generated: int = 0):
        m, ctx = self.m, list(context)
        k = min(int(k_max), MAX_ROWS - 1, int(m.cfg.max_context_len) - len(ctx))
        if k <= 0:
            return [], None
        if m.cfg.vocab_size != self.logits.shape[1]:
            raise ValueError("DraftModelProposer: the draft model's vocabulary changed")
        self._catch_up(ctx)
        tok, ids = ctx[-1], []
        for i in range(k):
            m.set_state_seq(self.seq, tok, len(ctx) - 1 + i)
            row = m.verify_step(self.seq, 1)[0:1]  # one row of this sequence: the batch-1 launches
            self.logits[i].copy_(row[0])
            if temperature > 0:
                tok = sampler.categorical_token(self._cat(row, temperature, [uniform_for(seed, DRAFT_STREAM + n_generated + i)]).cpu().numpy()[0])[0]
            else:
                tok = sampler.top1_token(self._top1(row).cpu().numpy()[0])
            self.done.append(ctx[-1] if i == 0 else ids[-1])
            ids.append(tok)
        return ids, self.logits[:k + 1]  # the verifier takes draft rows in the target's shape: k judged rows + the bonus row


def _refuse(model, top_k, top_p, min_p, frequency_penalty, presence_penalty, repetition_penalty, logit_bias):
    if top_k is not None and int(top_k) > 0:
        raise ValueError("speculative decoding: top_k > 0 is not supported (the stochastic rule needs the filtered distributions of speculative_target_probs)")
    if sampler.cut_active(top_p) or sampler.cut_active(min_p):
        raise ValueError("speculative decoding: top_p < 1 / min_p > 0 are not supported (the stochastic rule needs the filtered distributions)")
    if sampler.penalties_active(frequency_penalty, presence_penalty, repetition_penalty, logit_bias):
        raise ValueError("speculative decoding: penalties and logit bias are not supported")
    if getattr(model, "_comm", None) is not None or getattr(model, "_p2p", None) is not None or int(getattr(model.cfg, "tp_world_size", 1) or 1) > 1:
        raise ValueError("speculative decoding: a tensor-parallel model (comm / p2p route set) is not supported")


def generate_speculative(model, prompt, max_new_tokens: int, proposer, n_draft: int, temperature: float = 0.0, seed: int = 0, top_k=None, top_p: float = 1.0,
                         min_p: float = 0.0, frequency_penalty: float = 0.0, presence_penalty: float = 0.0, repetition_penalty: float = 1.0, logit_bias=None,
                         return_logits: bool = False, after_prompt=None):
    """Speculative decoding of sequence 0 on a `Llama` runner (decode engine): returns (tokens, stats) with stats = {"rounds", "proposed", "accepted"} (and "logits":
    the logits row each emitted token came from, with return_logits).  Per round: the proposer drafts k <= n_draft tokens; `verify_step` scores the anchor and the
    drafts in one step; `SpecVerify` judges them; `mrs_spec_advance` moves the decode state; ONE read-back of (n_accepted, out_tokens).  temperature 0 is greedy and
    lossless: ids and logits bits of a plain `decode_step` run.  k is clipped so that no row passes max_context_len - 1 and no token passes max_new_tokens or the
    model's tokens_out buffer.  The prompt goes through the prompt path in the decode engine's arithmetic (`prefill`, or `prefill_chunked` where that is not exact).
    `after_prompt`: called once, with no arguments, when the prompt is in the pages and before the first round (a timer's start: scripts/bench_speculative.py).
    Refuses (ValueError) top_k > 0, top_p < 1, min_p > 0, penalties, logit bias and a tensor-parallel model."""
    _refuse(model, top_k, top_p, min_p, frequency_penalty, presence_penalty, repetition_penalty, logit_bias)
    n_draft = int(n_draft)
    temperature = float(temperature)
    if n_draft < 0 or n_draft >= MAX_ROWS:
        raise ValueError(f"speculative decoding: n_draft must be in [0, {MAX_ROWS - 1}]")
    if not (np.isfinite(temperature) and temperature >= 0):
        raise ValueError("speculative decoding requires a finite temperature >= 0")
    prompt = [int(t) for t in prompt]
    cfg = model.cfg
    if not prompt or len(prompt) > cfg.max_context_len:
        raise ValueError("speculative decoding: the prompt must hold 1..max_context_len tokens")
    n_draft = min(n_draft, min(MAX_ROWS, int(cfg.max_batch)) - 1)
    verify = getattr(model, "_spec_verify", None)
    if verify is None or verify.vocab != cfg.vocab_size:
        verify = model._spec_verify = SpecVerify(cfg.vocab_size, model.device)
    proposer.reset()
    if len(prompt) > 1:
        if model.prefill_is_exact:
            model.prefill(prompt[:-1], 0)
        else:
            model.prefill_chunked(prompt[:-1], 0)
    model.set_state([prompt[-1]], [len(prompt) - 1])
    model.step_counter.zero_()
    if after_prompt is not None:
        after_prompt()
    toks, rows_out = [], []
    stats = {"rounds": 0, "proposed": 0, "accepted": 0}
    pos = len(prompt) - 1  # the anchor's position
    room = int(model.tokens_out.shape[1])
    while len(toks) < max_new_tokens and pos <= cfg.max_context_len - 1:
        k = min(n_draft, max_new_tokens - len(toks) - 1, cfg.max_context_len - 1 - pos, room - len(toks) - 1)
        if k < 0:
            break
        drafts, dlogits = proposer.propose(prompt + toks, k, temperature, seed, len(toks)) if k > 0 else ([], None)
        drafts = [int(d) for d in drafts][:k]
        k = len(drafts)
        logits = model.verify_step(0, k + 1, drafts)
        t0 = len(toks)
        us = [[uniform_for(seed, U0_STREAM + t0 + i), uniform_for(seed, t0 + i)] for i in range(k + 1)] if temperature > 0 else None
        if dlogits is not None and temperature > 0 and k > 0:
            if dlogits.shape[0] < k + 1:
                raise ValueError("speculative decoding: a proposer hands over k + 1 logits rows (the last one is the bonus row's place)")
            dlogits = dlogits[:k + 1]
        else:
            dlogits = None
        # draft_ids = the runner's id buffer from its second entry on: [d0 .. d(k-1)] and, for the bonus row, whatever follows (never read; the buffer has 9 entries)
        verify(logits, model.verify_ids_ptr + 4, [0, k + 1], temperature, us, dlogits)
        model.spec_advance(verify.n_accepted, verify.out_tokens, 0)
        res = verify.result.cpu().numpy()  # the round's one read-back
        n_acc = int(res[0])
        if n_acc < 0:
            raise ValueError("speculative decoding: the verifier met an unusable logits row (NaN / inf)")
        emitted = [int(t) for t in res[1:2 + n_acc]]
        if return_logits:
            rows_out.extend(logits[:n_acc + 1].clone().unbind(0))
        toks.extend(emitted)
        stats["rounds"] += 1
        stats["proposed"] += k
        stats["accepted"] += n_acc
        pos += n_acc + 1
    if return_logits:
        stats["logits"] = rows_out
    return toks, stats
