"""Temperature-sampled sequences through PagedEngine next to greedy ones: the draw of token j of a sequence depends on (its logits, its temperature,
uniform_for(its seed, j)) only, so a sequence that is chunk-prefilled, batched with others, preempted and recomputed generates exactly what it generates alone.
CPU: the fake runner (logits = a hash of the pages a row reads) and `categorical_host`; GPU: the real runner and the device categorical draw."""
import numpy as np
import pytest


class _FakeRunner:
    """The slice of mistralrs_amd.llama.Llama that PagedEngine drives (as in tests/test_scheduler.py): the logits are a hash of the token ids found IN THE PAGES of the
    positions 0 .. pos of the row's block table, so any mistake in block tables, slot mappings, chunk boundaries, preemption or recomputation changes them."""

    def __init__(self, num_blocks, block_size=8, max_batch=8, max_ctx=96, vocab=97):
        import torch
        from types import SimpleNamespace
        self.cfg = SimpleNamespace(block_size=block_size, max_batch=max_batch, max_context_len=max_ctx, vocab_size=vocab,
                                   max_blocks_per_seq=(max_ctx + block_size - 1) // block_size + 1)
        self.device = torch.device("cpu")
        self.block_tables = torch.zeros(max_batch, self.cfg.max_blocks_per_seq, dtype=torch.int32)
        self.pages = np.full(num_blocks * block_size, -1, dtype=np.int64)
        self.num_blocks = num_blocks

    def _slot(self, row, pos):
        bs = self.cfg.block_size
        return int(self.block_tables[row, pos // bs]) * bs + pos % bs

    def set_state(self, ids, positions):
        self._ids, self._pos = list(ids), list(positions)

    def forward_logits(self, b):
        import torch
        assert b == len(self._ids)
        for i in range(b):  # reshape_and_cache of every row first, then attention
            self.pages[self._slot(i, self._pos[i])] = self._ids[i]
        out = torch.empty(b, self.cfg.vocab_size)
        for i in range(b):
            ctx = [int(self.pages[self._slot(i, p)]) for p in range(self._pos[i] + 1)]
            assert -1 not in ctx, "a row read a page nobody wrote"
            g = np.random.default_rng(abs(hash(tuple(ctx))) % (2 ** 32))
            out[i] = torch.from_numpy(g.standard_normal(self.cfg.vocab_size).astype(np.float32))
        return out


def test_sampled_and_greedy_sequences_under_pool_pressure_on_a_fake_runner():
    """7 sequences on a pool that holds about three of them; the odd ones sampled at temperature 0.9 with their own seeds, the even ones greedy.  Preemptions occur;
    every sequence generates exactly what it generates alone."""
    import torch
    from mistralrs_amd import sampler
    from mistralrs_amd.kv_cache_manager import KVCacheManager
    from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
    lens = [(5, 9), (20, 12), (41, 6), (12, 20), (20, 7), (33, 5), (3, 30)]
    head = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26]  # two full 8-token blocks shared by some prompts
    prompts = [(head if i % 2 else []) + [(31 * i + 7 * j * j) % 90 for j in range(n)] for i, (n, _) in enumerate(lens)]
    temp = lambda i: 0.9 if i % 2 else None
    nb = 14
    m = _FakeRunner(nb)
    mgr = KVCacheManager(nb, 8, True, [0])
    sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16, max_decode_steps_before_prefill=3), mgr)
    seqs = [Sequence(id=i + 1, tokens=list(p), max_new_tokens=nn, temperature=temp(i), seed=100 + i) for i, (p, (_, nn)) in enumerate(zip(prompts, lens))]
    for s in seqs:
        sched.add_seq(s)
    eng = PagedEngine(m, sched)
    eng.run(max_steps=5000)
    assert all(s.state == "done" and len(s.generated) == nn for s, (_, nn) in zip(seqs, lens))
    assert eng.steps["prompt"] > len(seqs) and eng.steps["completion"] > 0 and eng.steps["preemptions"] > 0, eng.steps
    assert mgr.num_free_blocks() == mgr.num_usable_blocks()
    differs = 0
    for i, (s, p, (_, nn)) in enumerate(zip(seqs, prompts, lens)):
        solo = _FakeRunner(16)
        solo.block_tables[0] = torch.arange(1, 1 + solo.cfg.max_blocks_per_seq, dtype=torch.int32) % 16
        toks, lps, lg = list(p), [], None
        for pos in range(len(p) + nn - 1):
            solo.set_state([toks[pos]], [pos])
            lg = solo.forward_logits(1)[0]
            if pos >= len(p) - 1:
                if temp(i) is None:
                    toks.append(int(lg.argmax()))
                else:
                    tok, lp = sampler.categorical_host(lg.numpy(), np.float32(1.0 / temp(i)), sampler.uniform_for(100 + i, pos - (len(p) - 1)))
                    differs += tok != int(lg.argmax())
                    toks.append(tok)
                    lps.append(lp)
        assert toks[len(p):] == s.generated, (s.id, toks[len(p):], s.generated)
        assert torch.equal(lg, s.last_logits), s.id
        assert s.logprobs == lps and all(np.isfinite(lp) and lp <= 0 for lp in s.logprobs)
        assert len(s.logprobs) == (nn if temp(i) is not None else 0)
    assert differs > 0  # the sampled sequences did not just repeat the arg-max


def test_engine_raises_on_an_unusable_row():
    """a NaN in a sampled row's logits: no token is handed out"""
    import torch
    from mistralrs_amd.scheduler import PagedEngine, Sequence
    eng = PagedEngine(_FakeRunner(4), scheduler=None)
    seq = Sequence(id=1, tokens=[1, 2], temperature=0.7)
    lg = torch.zeros(1, 97)
    lg[0, 5] = float("nan")
    with pytest.raises(ValueError, match="invalid batched CUDA categorical output"):
        eng._finish_tokens([seq], lg)
    assert seq.generated == [] and seq.logprobs == []


@pytest.mark.gpu
def test_sampled_and_greedy_sequences_on_the_runner(oracle, dev, request):
    """The shapes of test_scheduler.py's bit-exact engine test, three sequences sampled (temperatures 0.8 / 1.0 / 1.3, own seeds) and three greedy: the scheduled run
    equals the solo run token for token (the logits are bit-identical, the device draw is a function of the row alone)."""
    import torch
    from mistralrs_amd import sampler
    from mistralrs_amd.kv_cache_manager import KVCacheManager
    from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
    from tests.test_dec_model import Q4KM, _mk
    if request.config.getoption("--host-emulation"):
        pytest.skip("~20 minutes on the host emulation; the bookkeeping runs on the fake runner in the CPU suite")
    lens = [(5, 6), (33, 8), (70, 6), (12, 14), (33, 7), (20, 6)]
    temps = [None, 0.8, None, 1.0, None, 1.3]
    cfg, w, m, cos, sin = _mk(oracle, dev, Q4KM(oracle), "bf16", max_batch=8, max_ctx=128, max_new=8)
    prompts = [[(1000 + 13 * i + 7 * j * j) % cfg.vocab_size for j in range(n)] for i, (n, _) in enumerate(lens)]
    pool = 7  # 32-token blocks: not enough for everyone at once
    mgr = KVCacheManager(pool, cfg.block_size, True, [0])
    assert pool <= m.num_blocks
    sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16, max_decode_steps_before_prefill=3), mgr)
    seqs = [Sequence(id=i + 1, tokens=list(p), max_new_tokens=nn, temperature=temps[i], seed=40 + i) for i, (p, (_, nn)) in enumerate(zip(prompts, lens))]
    for s in seqs:
        sched.add_seq(s)
    eng = PagedEngine(m, sched)
    eng.run(max_steps=4000)
    assert all(s.state == "done" and len(s.generated) == nn for s, (_, nn) in zip(seqs, lens))
    assert eng.steps["prompt"] > len(seqs) and eng.steps["completion"] > 0 and eng.steps["preemptions"] > 0, eng.steps
    assert mgr.num_free_blocks() == mgr.num_usable_blocks()
    cat = sampler.Categorical(cfg.vocab_size, dev)
    differs = 0
    for i, (s, p, (_, nn)) in enumerate(zip(seqs, prompts, lens)):
        cfg2, _, solo, _, _ = _mk(oracle, dev, Q4KM(oracle), "bf16", max_batch=8, max_ctx=128, max_new=8)
        toks, lps, lg = list(p), [], None
        for pos in range(len(p) + nn - 1):
            solo.set_state([toks[pos]], [pos])
            lg = solo.forward_logits(1)[0]
            if pos >= len(p) - 1:
                if temps[i] is None:
                    toks.append(int(lg.argmax()))
                else:
                    u = sampler.uniform_for(40 + i, pos - (len(p) - 1))
                    tok, lp = sampler.categorical_token(cat(lg.float().reshape(1, -1).contiguous(), temps[i], [u]).cpu().numpy()[0])
                    differs += tok != int(lg.argmax())
                    toks.append(tok)
                    lps.append(lp)
        assert toks[len(p):] == s.generated, (s.id, toks[len(p):], s.generated)
        assert torch.equal(lg, s.last_logits), s.id
        assert s.logprobs == lps and all(np.isfinite(lp) and lp <= 0 for lp in s.logprobs)
    assert differs > 0
