"""Sequences with a top_p / min_p cut through PagedEngine next to greedy and temperature-only ones: one launch mixes the three kinds; token j of a cut sequence
depends on (its logits, its parameters, uniform_for(its seed, j)) only, so a sequence that is batched, preempted and recomputed generates what it generates alone --
and the greedy and temperature-only sequences generate what they generate with no cut sequence around.  CPU: the fake runner and `nucleus_host`; GPU: the real
runner and the device draw.  `generate(..., full_vocab_cuts=True)` on the runner closes the file."""
import numpy as np
import pytest

from tests.test_zz_sampled_engine import _FakeRunner

# (temperature, top_p, min_p) by sequence index: greedy, temperature-only, top-p, min-p, greedy with inactive cut values, temperature-only, both cuts
KINDS = [(None, None, None), (0.9, None, None), (0.8, 0.9, None), (1.3, None, 0.1), (None, 1.0, 0.0), (1.2, None, None), (1.0, 0.5, 0.05)]


def in_nucleus(x, temp, top_p, min_p, tok):
    """float64: the token survives both cuts, with f32 rounding (2^-20 relative: 8 ulps) allowed at the edge of each"""
    z = x.astype(np.float64) * np.float64(np.float32(1.0 / temp))
    w = np.exp(z - z.max())
    slack = 2.0 ** -20
    ok = True
    if top_p is not None and 0 < top_p < 1:
        ok = ok and w[x > x[tok]].sum() / w.sum() < top_p * (1 + slack)
    if min_p is not None and 0 < min_p < 1:
        ok = ok and w[tok] > min_p * (1 - slack)
    return bool(ok)


def draw_solo(sampler, lg, kind, seed, j, dev_nuc=None, dev_cat=None):
    temp, top_p, min_p = kind
    if temp is None:
        return int(lg.argmax()), None
    u = sampler.uniform_for(seed, j)
    cut = sampler.cut_active(top_p) or sampler.cut_active(min_p)
    tp, mp = (top_p if sampler.cut_active(top_p) else 1.0), (min_p if sampler.cut_active(min_p) else 0.0)
    if dev_nuc is None:
        x = lg.float().numpy()
        return sampler.nucleus_host(x, np.float32(1.0 / temp), u, tp, mp)[:2] if cut else sampler.categorical_host(x, np.float32(1.0 / temp), u)
    x = lg.float().reshape(1, -1).contiguous()
    return sampler.nucleus_token(dev_nuc(x, temp, [u], tp, mp).cpu().numpy()[0]) if cut else sampler.categorical_token(dev_cat(x, temp, [u]).cpu().numpy()[0])


def run_mixed(make_runner, solo_runner, lens, prompts, pool, block, dev_nuc=None, dev_cat=None, pressure=True):
    """pressure: the pool holds about three sequences, a preemption must occur; else the pool holds all, and one launch must mix the three kinds"""
    import torch
    from mistralrs_amd import sampler
    from mistralrs_amd.kv_cache_manager import KVCacheManager
    from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
    m = make_runner()
    mgr = KVCacheManager(pool, block, True, [0])
    sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16, max_decode_steps_before_prefill=3), mgr)
    seqs = [Sequence(id=i + 1, tokens=list(p), max_new_tokens=nn, temperature=KINDS[i][0], top_p=KINDS[i][1], min_p=KINDS[i][2], seed=70 + i)
            for i, (p, (_, nn)) in enumerate(zip(prompts, lens))]
    for s in seqs:
        sched.add_seq(s)
    eng = PagedEngine(m, sched)
    kinds_per_launch = []
    finish = eng._finish_tokens
    eng._finish_tokens = lambda rows, lg: (kinds_per_launch.append({"greedy" if s.temperature is None else ("cut" if sampler.cut_active(s.top_p) or sampler.cut_active(s.min_p) else "temp")
                                                                    for s in rows}), finish(rows, lg))[1]
    eng.run(max_steps=5000)
    assert all(s.state == "done" and len(s.generated) == nn for s, (_, nn) in zip(seqs, lens))
    assert eng.steps["completion"] > 0 and (eng.steps["preemptions"] > 0 or not pressure), eng.steps
    assert mgr.num_free_blocks() == mgr.num_usable_blocks()
    assert pressure or any(k == {"greedy", "temp", "cut"} for k in kinds_per_launch), "no launch mixed greedy, temperature-only and cut rows"
    cut_differs = 0
    for i, (s, p, (_, nn)) in enumerate(zip(seqs, prompts, lens)):
        solo = solo_runner()
        toks, lps, lg = list(p), [], None
        for pos in range(len(p) + nn - 1):
            solo.set_state([toks[pos]], [pos])
            lg = solo.forward_logits(1)[0]
            if pos >= len(p) - 1:
                tok, lp = draw_solo(sampler, lg, KINDS[i], 70 + i, pos - (len(p) - 1), dev_nuc, dev_cat)
                temp, top_p, min_p = KINDS[i]
                if temp is not None:
                    assert in_nucleus(lg.float().cpu().numpy().reshape(-1), temp, top_p, min_p, tok), (s.id, pos, tok)
                    lps.append(lp)
                    cut_differs += tok != int(lg.argmax())
                toks.append(tok)
        assert toks[len(p):] == s.generated, (s.id, toks[len(p):], s.generated)
        assert torch.equal(lg, s.last_logits), s.id
        assert s.logprobs == lps and all(np.isfinite(lp) and lp <= 0 for lp in s.logprobs)
    assert cut_differs > 0


def test_cut_temperature_and_greedy_sequences_under_pool_pressure_on_a_fake_runner():
    import torch
    lens = [(5, 9), (20, 12), (41, 6), (12, 20), (20, 7), (33, 5), (3, 30)]
    head = list(range(11, 27))
    prompts = [(head if i % 2 else []) + [(31 * i + 7 * j * j) % 90 for j in range(n)] for i, (n, _) in enumerate(lens)]

    def solo():
        r = _FakeRunner(16)
        r.block_tables[0] = torch.arange(1, 1 + r.cfg.max_blocks_per_seq, dtype=torch.int32) % 16
        return r
    run_mixed(lambda: _FakeRunner(14), solo, lens, prompts, 14, 8)
    run_mixed(lambda: _FakeRunner(64), solo, lens, prompts, 64, 8, pressure=False)


def test_a_cut_without_a_temperature_is_refused_at_submission():
    import torch
    from mistralrs_amd.kv_cache_manager import KVCacheManager
    from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
    sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16), KVCacheManager(4, 8, True, [0]))
    for kw in (dict(top_p=0.9), dict(min_p=0.1)):
        with pytest.raises(ValueError, match="need a temperature"):
            sched.add_seq(Sequence(id=1, tokens=[1, 2], **kw))
        with pytest.raises(ValueError, match="need a temperature"):
            PagedEngine(_FakeRunner(4), scheduler=None)._finish_tokens([Sequence(id=1, tokens=[1, 2], **kw)], torch.zeros(1, 97))
    sched.add_seq(Sequence(id=2, tokens=[1, 2], top_p=1.0, min_p=0.0))  # inactive values are no cut
    seq = Sequence(id=3, tokens=[1, 2], temperature=0.7, top_p=0.9)
    lg = torch.zeros(1, 97)
    lg[0, 5] = float("nan")
    with pytest.raises(ValueError, match="invalid batched nucleus output"):
        PagedEngine(_FakeRunner(4), scheduler=None)._finish_tokens([seq], lg)
    assert seq.generated == [] and seq.logprobs == []


@pytest.mark.gpu
def test_cut_temperature_and_greedy_sequences_on_the_runner(oracle, dev, request):
    from mistralrs_amd import sampler
    from tests.test_dec_model import Q4KM, _mk
    if request.config.getoption("--host-emulation"):
        pytest.skip("minutes on the host emulation; the bookkeeping runs on the fake runner in the CPU suite")
    lens = [(5, 6), (33, 8), (70, 6), (12, 14), (33, 7), (20, 6), (9, 8)]
    mk = lambda: _mk(oracle, dev, Q4KM(oracle), "bf16", max_batch=8, max_ctx=128, max_new=8)
    cfg, w, m, cos, sin = mk()
    prompts = [[(1000 + 13 * i + 7 * j * j) % cfg.vocab_size for j in range(n)] for i, (n, _) in enumerate(lens)]
    assert 7 <= m.num_blocks
    nuc, cat = sampler.Nucleus(cfg.vocab_size, dev), sampler.Categorical(cfg.vocab_size, dev)
    run_mixed(lambda: m, lambda: mk()[2], lens, prompts, 7, cfg.block_size, nuc, cat)
    # the pool holds all four short sequences (one 32-token block each): they decode side by side, so one launch mixes greedy, temperature-only and cut rows
    short = [(5, 8), (6, 8), (7, 8), (5, 8)]
    run_mixed(lambda: mk()[2], lambda: mk()[2], short, [p[:n] for p, (n, _) in zip(prompts, short)], 7, cfg.block_size, nuc, cat, pressure=False)


@pytest.mark.gpu
def test_generate_with_full_vocab_cuts_on_the_runner(oracle, dev):
    from mistralrs_amd import sampler
    from tests.test_dec_model import Q4KM, _mk
    cfg, w, m, cos, sin = _mk(oracle, dev, Q4KM(oracle), "bf16")
    prompt = [(1000 + 7 * i) % cfg.vocab_size for i in range(12)]
    a = sampler.generate(m, prompt, 6, top_k=0, temperature=1.5, top_p=0.9, seed=5, full_vocab_cuts=True)
    assert a == sampler.generate(m, prompt, 6, top_k=None, temperature=1.5, top_p=0.9, seed=5, full_vocab_cuts=True) and len(a[0]) == 6
    lg = m.prefill(prompt, 0)
    for i, (tok, p) in enumerate(zip(*a)):
        x = lg.float().reshape(-1).cpu().numpy()
        assert in_nucleus(x, 1.5, 0.9, None, tok), (i, tok)
        z = x.astype(np.float64) * np.float64(np.float32(1.0 / 1.5))
        lp = z[tok] - z.max() - np.log(np.exp(z - z.max()).sum())
        assert 0 < p <= 1 and abs(np.log(p) - lp) <= 2e-6 * (1 + abs(lp)) + 1e-7
        m.set_state([tok], [len(prompt) + i])
        lg = m.forward_logits(1)[0]
    b = sampler.generate(m, prompt, 3, top_k=0, temperature=1.5, min_p=0.2, seed=5, full_vocab_cuts=True)
    assert len(b[0]) == 3
    with pytest.raises(ValueError, match="top_k"):
        sampler.generate(m, prompt, 2, top_k=0, top_p=0.9)
