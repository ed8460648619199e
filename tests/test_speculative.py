"""Speculative decoding on the runner (mistralrs_amd/speculative.py): greedy rounds are LOSSLESS -- the ids and the logits bits of a plain `decode_step` run, whatever the
proposer does -- because the batched decode launches of the verify step produce the batch-1 step's bits.  Smallest engine model of tests/test_dec_model.py (2 layers,
Q4_K / Q6_K)."""
import numpy as np
import pytest

from tests.test_dec_model import Q4KM, _mk

pytestmark = pytest.mark.gpu
NEW = 48


def _prompt(cfg, n=40):
    return [(1000 + 7 * i) % cfg.vocab_size for i in range(n)]


def _plain(m, prompt, new):
    """token-by-token: (ids, the logits row each id came from)"""
    for pos, t in enumerate(prompt[:-1]):
        m.set_state([t], [pos])
        m.forward_logits(1)
    m.set_state([prompt[-1]], [len(prompt) - 1])
    m.step_counter.zero_()
    new = min(new, m.cfg.max_context_len - len(prompt) + 1)
    rows = []
    for _ in range(new):
        m.decode_step(1)
        rows.append(m.logits[0].clone())
    return m.tokens_out[0, :new].cpu().numpy().tolist(), rows


class Replay:
    """proposes the plain run's own tokens; `wrong(j)` plants an error into the j-th draft it ever made"""

    def __init__(self, plain, vocab, wrong=lambda j: False):
        self.plain, self.vocab, self.wrong = plain, vocab, wrong

    def reset(self):
        self.made = 0

    def propose(self, context, k_max, temperature=0.0, seed=0, n_generated=0):
        out = []
        for t in self.plain[n_generated:n_generated + k_max]:
            out.append((t + 1) % self.vocab if self.wrong(self.made) else t)
            self.made += 1
        return out, None


def _pages(m, length, seq=0):
    """K / V of the positions below `length` of sequence `seq`, layer by layer"""
    bs, out = m.cfg.block_size, []
    for kc, vc in zip(m.key_caches, m.value_caches):
        for b in range((length + bs - 1) // bs):
            blk, cnt = int(m.block_tables[seq, b].item()), min(bs, length - b * bs)
            out += [kc[blk][:, :, :cnt, :].clone(), vc[blk][:, :, :cnt].clone()]
    return out


def _check_lossless(m_plain, m, prompt, plain, rows, proposer, n_draft):
    import torch
    from mistralrs_amd import speculative
    toks, st = speculative.generate_speculative(m, prompt, NEW, proposer, n_draft, return_logits=True)
    assert toks == plain, (n_draft, toks, plain)
    for i, (a, b) in enumerate(zip(st["logits"], rows)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"token {i}: the logits row differs from the plain run's"
    assert st["accepted"] + st["rounds"] == len(toks) and st["accepted"] <= st["proposed"]
    assert int(m.step_counter.item()) == len(toks) and m.tokens_out[0, :len(toks)].cpu().numpy().tolist() == toks
    for a, b in zip(_pages(m, len(prompt) + len(toks) - 1), _pages(m_plain, len(prompt) + len(toks) - 1)):
        assert torch.equal(a, b), "K/V pages differ from the plain run's"
    return st


@pytest.fixture(scope="module")
def pair(oracle, dev):
    cfg, _, m_plain, _, _ = _mk(oracle, dev, Q4KM(oracle), "bf16", max_batch=8)
    _, _, m, _, _ = _mk(oracle, dev, Q4KM(oracle), "bf16", max_batch=8)
    prompt = _prompt(cfg)
    plain, rows = _plain(m_plain, prompt, NEW)
    return cfg, m_plain, m, prompt, plain, rows


@pytest.mark.parametrize("n_draft", [1, 2, 4, 7])
def test_lossless_greedy(pair, n_draft):
    """2 rows stay on the vector-ALU route, 3 and more go through the matrix cores, 8 rows is the maximum"""
    from mistralrs_amd import speculative
    cfg, m_plain, m, prompt, plain, rows = pair
    st = _check_lossless(m_plain, m, prompt, plain, rows, Replay(plain, cfg.vocab_size), n_draft)
    assert st["rounds"] == -(-NEW // (n_draft + 1)) and st["accepted"] == NEW - st["rounds"]
    st = _check_lossless(m_plain, m, prompt, plain, rows, Replay(plain, cfg.vocab_size, wrong=lambda j: True), n_draft)
    assert st["accepted"] == 0 and st["rounds"] == NEW
    st = _check_lossless(m_plain, m, prompt, plain, rows, Replay(plain, cfg.vocab_size, wrong=lambda j: j % 3 == 2), n_draft)
    assert 0 < st["accepted"] < st["proposed"] or n_draft == 1
    _check_lossless(m_plain, m, prompt, plain, rows, speculative.NGramProposer(3, n_draft), n_draft)


@pytest.mark.parametrize("case", ["straddle", "clipped", "f8e4m3", "window", "moe"])
def test_lossless_greedy_variants(oracle, dev, case):
    """a round that straddles positions 31 | 32; the last round clipped by max_context_len; FP8 pages; a sliding window of 16 behind a longer context; 4 experts"""
    kw = dict(clipped=dict(max_ctx=64), f8e4m3=dict(kv_dtype="f8e4m3"), window=dict(sliding_window=16), moe=dict(experts=4)).get(case, {})
    cfg, _, m_plain, _, _ = _mk(oracle, dev, Q4KM(oracle), **{"kv_dtype": "bf16", "max_batch": 8, **kw})
    _, _, m, _, _ = _mk(oracle, dev, Q4KM(oracle), **{"kv_dtype": "bf16", "max_batch": 8, **kw})
    prompt = _prompt(cfg, 29 if case == "straddle" else 40)  # anchor at 28: a 7-draft round covers 28 .. 35
    plain, rows = _plain(m_plain, prompt, NEW)
    assert len(plain) == (25 if case == "clipped" else NEW)
    st = _check_lossless(m_plain, m, prompt, plain, rows, Replay(plain, cfg.vocab_size, wrong=lambda j: j % 5 == 4), 7)
    assert st["accepted"] > 0


def test_draft_model_all_accepted(oracle, dev, pair):
    """the target's own weights as the draft: p == q bit for bit, so every draft is accepted at temperature 0 and at 0.8; seeds reproduce; greedy ids are the plain run's"""
    from mistralrs_amd import speculative
    cfg, m_plain, m, prompt, plain, rows = pair
    _, _, md, _, _ = _mk(oracle, dev, Q4KM(oracle), "bf16", max_batch=8)
    prop = speculative.DraftModelProposer(md)
    toks, st = speculative.generate_speculative(m, prompt, 24, prop, 4)
    assert toks == plain[:24] and st["accepted"] == st["proposed"] > 0
    a, sa = speculative.generate_speculative(m, prompt, 24, prop, 4, temperature=0.8, seed=5)
    b, sb = speculative.generate_speculative(m, prompt, 24, prop, 4, temperature=0.8, seed=5)
    assert a == b and len(a) == 24 and sa["accepted"] == sa["proposed"] > 0 and sa == sb
    c, _ = speculative.generate_speculative(m, prompt, 24, prop, 4, temperature=0.8, seed=6)
    assert c != a
    # the multi-row catch-up (inside generate_speculative the gap is at most one token): the proposer meets a context that is three tokens ahead of its pages
    prop.reset()
    assert prop.propose(prompt, 3)[0] == plain[:3] and prop.done == prompt + plain[:2]
    ids, rows_q = prop.propose(prompt + plain[:6], 3)  # pages end at plain[1]; plain[2:5] go through ONE 3-row step, then the drafts from the anchor plain[5]
    assert ids == plain[6:9] and prop.done == prompt + plain[:8] and rows_q.shape[0] == 4
    # ... and one that parted from its pages: the tokens after the common prefix are redone
    other = prompt + plain[:3] + [(plain[3] + 1) % cfg.vocab_size]
    ids2, _ = prop.propose(other, 2)
    assert prop.done[:len(other)] == other and len(ids2) == 2


def test_isolation_and_refusals(pair):
    """a speculative run on sequence 0 leaves a second sequence's block-table row and pages alone; what the path does not serve is refused"""
    import torch
    from mistralrs_amd import speculative
    cfg, m_plain, m, prompt, plain, rows = pair
    other = [(3 + 5 * i) % cfg.vocab_size for i in range(20)]
    m.prefill(other, 0, seq=1)
    before_bt, before = m.block_tables.clone(), _pages(m, 20, seq=1)
    toks, _ = speculative.generate_speculative(m, prompt, NEW, Replay(plain, cfg.vocab_size, wrong=lambda j: j % 4 == 3), 7)
    assert toks == plain
    assert torch.equal(m.block_tables, before_bt) and all(torch.equal(a, b) for a, b in zip(before, _pages(m, 20, seq=1)))
    rp = Replay(plain, cfg.vocab_size)
    for kw in (dict(top_k=4), dict(top_p=0.9), dict(min_p=0.1), dict(frequency_penalty=0.5), dict(presence_penalty=0.5), dict(repetition_penalty=1.1),
               dict(logit_bias={3: 1.0})):
        with pytest.raises(ValueError, match="speculative decoding"):
            speculative.generate_speculative(m, prompt, 4, rp, 2, **kw)
    m._comm = object()
    try:
        with pytest.raises(ValueError, match="tensor-parallel"):
            speculative.generate_speculative(m, prompt, 4, rp, 2)
    finally:
        m._comm = None
    with pytest.raises(ValueError):
        speculative.generate_speculative(m, prompt, 4, rp, 8)
    with pytest.raises(ValueError):
        m.verify_step(0, 9, [0] * 8)
