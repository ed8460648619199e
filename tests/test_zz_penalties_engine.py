"""Sequences with penalties or a logit bias through PagedEngine next to plain greedy, temperature-only and cut ones: one launch mixes penalized and plain rows; token j of a
sequence depends on (its logits, its own token history, its parameters, uniform_for(its seed, j)) only, so a sequence that is batched, preempted and recomputed generates
what it generates alone -- re-derived here position by position with `penalties_host` (CPU) or a one-row `Penalties` (GPU) in front of the existing rules -- and the plain
sequences generate what they generate with no penalized sequence around.  `sampler.generate` with the four keywords closes the file."""
import numpy as np
import pytest

from tests.test_zz_nucleus_engine import draw_solo
from tests.test_zz_sampled_engine import _FakeRunner

# by sequence index: (temperature, top_p, min_p), then frequency / presence / repetition penalty and the bias
KINDS = [(None, None, None), (None, None, None), (0.9, None, None), (0.8, 0.9, None), (1.2, None, None), (1.3, None, 0.1), (None, None, None)]
PENS = [{}, dict(repetition_penalty=1.25), dict(frequency_penalty=0.5), dict(presence_penalty=0.5, logit_bias={3: 2.0, 50: -1.5, 1000003: 4.0}), {},
        dict(frequency_penalty=0.25, presence_penalty=0.125, repetition_penalty=1.5), dict(logit_bias={7: 3.0, 11: -2.0, 60: 0.0})]


def run_mixed(make_runner, solo_runner, lens, prompts, pool, block, kinds=KINDS, pens=PENS, dev=None, pressure=True):
    """pressure: the pool holds about three sequences, a preemption must occur; else the pool holds all, and one launch must mix penalized and plain rows"""
    import torch
    from mistralrs_amd import sampler
    from mistralrs_amd.kv_cache_manager import KVCacheManager
    from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
    m = make_runner()
    mgr = KVCacheManager(pool, block, True, [0])
    sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16, max_decode_steps_before_prefill=3), mgr)
    seqs = [Sequence(id=i + 1, tokens=list(p), max_new_tokens=nn, temperature=kinds[i][0], top_p=kinds[i][1], min_p=kinds[i][2], seed=70 + i, **pens[i])
            for i, (p, (_, nn)) in enumerate(zip(prompts, lens))]
    for s in seqs:
        sched.add_seq(s)
    eng = PagedEngine(m, sched)
    active = lambda s: sampler.penalties_active(s.frequency_penalty, s.presence_penalty, s.repetition_penalty, s.logit_bias)
    kinds_per_launch = []
    finish = eng._finish_tokens
    eng._finish_tokens = lambda rows, lg: (kinds_per_launch.append({"penalized" if active(s) else "plain" for s in rows}), finish(rows, lg))[1]
    eng.run(max_steps=5000)
    assert all(s.state == "done" and len(s.generated) == nn for s, (_, nn) in zip(seqs, lens))
    assert eng.steps["completion"] > 0 and (eng.steps["preemptions"] > 0 or not pressure), eng.steps
    assert mgr.num_free_blocks() == mgr.num_usable_blocks()
    assert pressure or any(k == {"penalized", "plain"} for k in kinds_per_launch), "no launch mixed penalized and plain rows"
    assert (sampler.Penalties in eng._draws) == (dev is not None)
    vocab = m.cfg.vocab_size
    ws = None if dev is None else (sampler.Penalties(vocab, dev, max_context=256), sampler.Nucleus(vocab, dev), sampler.Categorical(vocab, dev))
    moved = 0
    for i, (s, p, (_, nn)) in enumerate(zip(seqs, prompts, lens)):
        solo = solo_runner()
        toks, lps, lg = list(p), [], None
        for pos in range(len(p) + nn - 1):
            solo.set_state([toks[pos]], [pos])
            lg = solo.forward_logits(1)[0]
            if pos >= len(p) - 1:
                row = lg
                if pens[i] and ws is None:
                    row = torch.from_numpy(sampler.penalties_host(lg.float().numpy(), toks, len(p), **pens[i]))
                elif pens[i]:
                    row = ws[0](lg.float().reshape(1, -1).contiguous(), [toks], len(p), **pens[i])[0].clone()
                tok, lp = draw_solo(sampler, row, kinds[i], 70 + i, pos - (len(p) - 1), *(() if ws is None else ws[1:]))
                moved += not torch.equal(row.cpu(), lg.float().cpu())
                if kinds[i][0] is not None:
                    lps.append(lp)
                toks.append(tok)
        assert toks[len(p):] == s.generated, (s.id, toks[len(p):], s.generated)
        assert torch.equal(lg, s.last_logits), s.id  # the RAW model row, not the sampler's input
        assert s.logprobs == lps and all(np.isfinite(lp) and lp <= 0 for lp in s.logprobs)
    assert moved > 0, "no penalty changed a row: the re-derivation would show nothing"
    return seqs


LENS = [(5, 9), (20, 12), (41, 6), (12, 20), (20, 7), (33, 5), (3, 30)]
HEAD = list(range(11, 27))
PROMPTS = [(HEAD if i % 2 else []) + [(31 * i + 7 * j * j) % 90 for j in range(n)] for i, (n, _) in enumerate(LENS)]


def _solo():
    import torch
    r = _FakeRunner(16)
    r.block_tables[0] = torch.arange(1, 1 + r.cfg.max_blocks_per_seq, dtype=torch.int32) % 16
    return r


def test_penalized_and_plain_sequences_under_pool_pressure_on_a_fake_runner():
    run_mixed(lambda: _FakeRunner(14), _solo, LENS, PROMPTS, 14, 8)


def test_penalized_and_plain_sequences_side_by_side_on_a_fake_runner():
    run_mixed(lambda: _FakeRunner(64), _solo, LENS, PROMPTS, 64, 8, pressure=False)


def test_plain_sequences_generate_the_same_with_no_penalized_sequence_around():
    """the two plain sequences of the mix, run again with every penalty taken out of the other five: same tokens, same logprobs, and no call of the penalties at all"""
    with_pens = run_mixed(lambda: _FakeRunner(64), _solo, LENS, PROMPTS, 64, 8, pressure=False)
    import mistralrs_amd.sampler as sampler
    calls = []
    real = sampler.penalties_host
    sampler.penalties_host = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        from mistralrs_amd.kv_cache_manager import KVCacheManager
        from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
        sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16, max_decode_steps_before_prefill=3), KVCacheManager(64, 8, True, [0]))
        seqs = [Sequence(id=i + 1, tokens=list(p), max_new_tokens=nn, temperature=KINDS[i][0], top_p=KINDS[i][1], min_p=KINDS[i][2], seed=70 + i)
                for i, (p, (_, nn)) in enumerate(zip(PROMPTS, LENS))]
        for s in seqs:
            sched.add_seq(s)
        PagedEngine(_FakeRunner(64), sched).run(max_steps=5000)
    finally:
        sampler.penalties_host = real
    assert not calls, "a launch without a penalized row went through the penalties"
    for i in (0, 4):
        assert seqs[i].generated == with_pens[i].generated and seqs[i].logprobs == with_pens[i].logprobs
    assert any(seqs[i].generated != with_pens[i].generated for i in (1, 2, 3, 5, 6))


def _one(seq_kw, new=30, prompt=(4, 9, 2)):
    from mistralrs_amd.kv_cache_manager import KVCacheManager
    from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
    sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16), KVCacheManager(64, 8, True, [0]))
    seq = Sequence(id=1, tokens=list(prompt), max_new_tokens=new, **seq_kw)
    sched.add_seq(seq)
    PagedEngine(_FakeRunner(64), sched).run(max_steps=5000)
    assert len(seq.generated) == new
    return seq.generated


def test_effects_on_a_vocabulary_of_97():
    plain = _one({})
    assert len(set(plain)) < 30, "N(0, 1) rows over 97 tokens repeat within 30 greedy tokens: the next assertion would show nothing otherwise"
    assert len(set(_one(dict(presence_penalty=64.0)))) == 30  # a generated token is 64 below where it was, for good
    for t in (0, 42, 96):
        assert _one(dict(logit_bias={t: 100.0}), new=8) == [t] * 8
        assert _one(dict(logit_bias={t: 100.0}, temperature=0.7, seed=3), new=8) == [t] * 8  # the draw sees the biased row too
    a = plain[0]
    assert _one(dict(logit_bias={a: -100.0}), new=2)[0] != a


def test_invalid_penalties_are_refused_at_submission_and_at_the_draw():
    import torch
    from mistralrs_amd.kv_cache_manager import KVCacheManager
    from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
    sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16), KVCacheManager(4, 8, True, [0]))
    bad = [dict(frequency_penalty=float("nan")), dict(presence_penalty=float("inf")), dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0),
           dict(repetition_penalty=float("nan")), dict(logit_bias={-3: 1.0}), dict(logit_bias={2.5: 1.0}), dict(logit_bias={3: float("nan")}), dict(logit_bias={3: float("inf")})]
    for kw in bad:
        for temp in (None, 0.8):
            with pytest.raises(ValueError, match=r"^penalties: "):
                sched.add_seq(Sequence(id=1, tokens=[1, 2], temperature=temp, **kw))
            seq = Sequence(id=1, tokens=[1, 2], temperature=temp, **kw)
            other = Sequence(id=2, tokens=[3, 4], repetition_penalty=1.5)
            with pytest.raises(ValueError, match=r"^penalties: "):
                PagedEngine(_FakeRunner(4), scheduler=None)._finish_tokens([other, seq], torch.zeros(2, 97))
            assert seq.generated == [] and seq.logprobs == [] and other.generated == [] and seq.tokens == [1, 2] and other.tokens == [3, 4]
    assert sched.waiting_len() == 0
    sched.add_seq(Sequence(id=3, tokens=[1, 2], frequency_penalty=0.0, presence_penalty=0.0, repetition_penalty=1.0, logit_bias={}))  # inactive values
    sched.add_seq(Sequence(id=4, tokens=[1, 2], repetition_penalty=1.1))  # a penalty on a greedy sequence is allowed
    assert sched.waiting_len() == 2


@pytest.mark.gpu
def test_penalized_and_plain_sequences_on_the_runner(oracle, dev, request):
    from tests.test_dec_model import Q4KM, _mk
    if request.config.getoption("--host-emulation"):
        pytest.skip("minutes on the host emulation; the bookkeeping runs on the fake runner in the CPU suite")
    lens = [(5, 6), (33, 8), (70, 6), (12, 14), (33, 7), (20, 6), (9, 8)]
    mk = lambda: _mk(oracle, dev, Q4KM(oracle), "bf16", max_batch=8, max_ctx=128, max_new=8)
    cfg, w, m, cos, sin = mk()
    prompts = [[(1000 + 13 * i + 7 * j * j) % cfg.vocab_size for j in range(n)] for i, (n, _) in enumerate(lens)]
    assert 7 <= m.num_blocks
    run_mixed(lambda: m, lambda: mk()[2], lens, prompts, 7, cfg.block_size, dev=dev)
    # the pool holds all four short sequences (one 32-token block each): greedy with a repetition penalty, temperature with a frequency penalty, top-p with a presence
    # penalty and a bias, plain greedy -- they decode side by side, so one launch mixes penalized and plain rows
    short = [(5, 8), (6, 8), (7, 8), (5, 8)]
    pick = [1, 2, 3, 0]
    run_mixed(lambda: mk()[2], lambda: mk()[2], short, [prompts[i][:n] for i, (n, _) in zip(pick, short)], 7, cfg.block_size, kinds=[KINDS[i] for i in pick],
              pens=[PENS[i] for i in pick], dev=dev, pressure=False)


def _manual(sampler, m, prompt, n, top_k, seed, temperature, pen_kw):
    """generate()'s loop written out: `Penalties` (when pen_kw) in front of the workspace of the mode"""
    vocab = int(m.cfg.vocab_size)
    ws = sampler.Categorical(vocab, m.device) if top_k == 0 else (sampler.Top1(vocab, m.device) if top_k == 1 else sampler.TopK(vocab, top_k, m.device))
    pen = sampler.Penalties(vocab, m.device, max_context=len(prompt) + n) if pen_kw else None
    rng = np.random.default_rng(seed)
    logits = m.prefill(list(prompt), 0).float().reshape(1, -1)
    toks, probs = [], []
    for i in range(n):
        row = logits.contiguous()
        if pen is not None:
            row = pen(row, [list(prompt) + toks], len(prompt), **pen_kw)
        if top_k == 0:
            tok, lp = sampler.categorical_token(ws(row, temperature, [sampler.uniform_for(seed, i)]).cpu().numpy()[0])
            p = min(1.0, float(np.exp(lp)))
        elif top_k == 1:
            tok, p = sampler.top1_token(ws(row).cpu().numpy()[0]), 1.0
        else:
            tok, p = sampler.sample(ws(row, temperature).cpu().numpy()[0], ws.k, temperature, 1.0, 0.0, rng)
        toks.append(tok)
        probs.append(p)
        if i + 1 < n:
            m.set_state([tok], [len(prompt) + i])
            logits = m.forward_logits(1)[0:1].float()
    return toks, probs


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [0, 1, 40])
def test_generate_with_penalties_on_the_runner(oracle, dev, top_k):
    from mistralrs_amd import sampler
    from tests.test_dec_model import Q4KM, _mk
    cfg, w, m, cos, sin = _mk(oracle, dev, Q4KM(oracle), "bf16")
    prompt = [(1000 + 7 * i) % cfg.vocab_size for i in range(12)]
    n, temp = 5, 1.5
    plain = sampler.generate(m, prompt, n, top_k=top_k, temperature=temp, seed=5)
    assert plain == _manual(sampler, m, prompt, n, top_k, 5, temp, None)  # the defaults: the loop without Penalties
    first = plain[0][0]
    differs = 0
    for kw in (dict(frequency_penalty=1.5), dict(presence_penalty=2.0), dict(repetition_penalty=1.8), dict(logit_bias={first: -50.0, prompt[0]: 3.0})):
        a = sampler.generate(m, prompt, n, top_k=top_k, temperature=temp, seed=5, **kw)
        assert a == sampler.generate(m, prompt, n, top_k=top_k, temperature=temp, seed=5, **kw) and len(a[0]) == n  # deterministic for a seed
        assert a == _manual(sampler, m, prompt, n, top_k, 5, temp, kw), kw
        differs += a != plain
    assert differs > 0 and sampler.generate(m, prompt, n, top_k=top_k, temperature=temp, seed=5, logit_bias={first: -50.0})[0][0] != first
    with pytest.raises(ValueError, match=r"^penalties: "):
        sampler.generate(m, prompt, 2, top_k=top_k, repetition_penalty=0.0)
