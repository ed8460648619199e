"""FP8 (E4M3) KV pages through the runner (Llama(kv_dtype="f8e4m3"), host/runtime.cpp): the 2-layer model of tests/test_dec_model.py with uint8 pages and static
per-layer scales.  Bit for bit: prefill == token-by-token decode (logits and page bytes) == LlamaRef(mode="engine") with the FP8 round trip as its KV rounding; two-chunk
prefill == one pass; batched steps == single steps; the captured (chained) graph == eager steps; PagedEngine with a preemption == plain greedy decoding.  And what
refuses FP8 pages says so."""
import ctypes as C

import numpy as np
import pytest

from tests.test_dec_model import Q4KM, _mk

pytestmark = pytest.mark.gpu
F8 = "f8e4m3"


def _fp8_round_trip(O, scale):
    s = np.float32(scale)
    return lambda x, dt: (O.fp8_e4m3_decode(O.fp8_e4m3_encode(np.asarray(x, np.float32) / s)) * s).astype(np.float32)


@pytest.mark.parametrize("case", ["one-scale-oracle", "unit-scales-oracle", "distinct-scales", "moe4"])
def test_prefill_equals_decode_equals_oracle_on_fp8_pages(oracle, dev, request, monkeypatch, case):
    """prefill(prompt) leaves the SAME page bytes and returns the SAME logits as decoding the prompt token by token; the same prompt in two chunks (the second starts at
    start_pos > 0 and attends the first's pages) too; decoding on from the prefilled pages matches.  With one value for both scales all of it equals
    LlamaRef(mode="engine") whose KV rounding is the FP8 round trip (llama_ref._round gets no hint whether it rounds K or V); distinct per-layer scales and the sparse-MoE
    model (its oracle is an f64 restatement) hold prefill == decode."""
    import torch
    from oracle import llama_ref
    emu = request.config.getoption("--host-emulation")
    n_prompt, n_more = (9, 2) if emu else (70, 12)
    experts = 4 if case == "moe4" else 0
    mk = lambda: _mk(oracle, dev, Q4KM(oracle), F8, experts=experts)[2]
    cfg, w, m1, cos, sin = _mk(oracle, dev, Q4KM(oracle), F8, experts=experts)
    m2, m3 = mk(), mk()
    models = (m1, m2, m3)
    assert m1.prefill_is_exact and m1.key_caches[0].dtype == torch.uint8 and m1.key_caches[0].shape[-1] == 16
    ref = None
    if case == "one-scale-oracle":
        for m in models:
            m.set_kv_scales(0.05, 0.05)
        monkeypatch.setattr(llama_ref, "_round", _fp8_round_trip(oracle, 0.05))
    elif case == "unit-scales-oracle":  # the default: the reference's uncalibrated cache
        monkeypatch.setattr(llama_ref, "_round", _fp8_round_trip(oracle, 1.0))
    else:
        for m in models:
            m.set_kv_scales([0.037, 0.05], [0.11, 0.2])
    if case.endswith("oracle"):
        ref = llama_ref.LlamaRef(cfg, w, cos, sin, mode="engine", kv_dtype=F8)
    prompt = [(1000 + 37 * i) % cfg.vocab_size for i in range(n_prompt)]
    lp = m1.prefill(prompt, 0).float().cpu().numpy()
    for pos, t in enumerate(prompt):
        m2.set_state([t], [pos])
        ld = m2.forward_logits(1)[0].float().cpu().numpy()
        assert ref is None or np.array_equal(ld, ref.step(t, pos)), f"decode position {pos} differs from the engine-order oracle"
    assert np.array_equal(lp, ld), f"prefill logits differ from token-by-token decode: max |d| = {float(np.abs(lp - ld).max()):.3e}"
    cut = n_prompt // 2 + 1
    m3.prefill(prompt[:cut], 0)
    lc = m3.prefill(prompt[cut:], cut).float().cpu().numpy()
    assert np.array_equal(lc, lp), "two-chunk prefill differs from the one-pass prefill"
    for layer in range(cfg.num_layers):
        for name, caches in (("K", [m.key_caches[layer] for m in models]), ("V", [m.value_caches[layer] for m in models])):
            assert int(caches[0].count_nonzero()) > 0
            assert torch.equal(caches[0], caches[1]), f"layer {layer}: {name} page bytes written by prefill != bytes written by decode"
            assert torch.equal(caches[0], caches[2]), f"layer {layer}: {name} page bytes of the chunked prefill differ"
    tok = int(lp.argmax())
    for pos in range(n_prompt, n_prompt + n_more):
        m1.set_state([tok], [pos])
        got = m1.forward_logits(1)[0].float().cpu().numpy()
        if ref is not None:
            assert np.array_equal(got, ref.step(tok, pos)), f"position {pos} after the prefill differs from the engine-order oracle"
        else:
            m2.set_state([tok], [pos])
            assert np.array_equal(got, m2.forward_logits(1)[0].float().cpu().numpy()), f"position {pos}: decoding on from prefilled pages differs"
        tok = int(got.argmax())


def test_sliding_window_prefill_equals_decode_on_fp8_pages(oracle, dev, request):
    """window 40, prompt past the window, second chunk at start_pos > 0: prefill == token-by-token decode, logits and page bytes"""
    import torch
    emu = request.config.getoption("--host-emulation")
    if emu:
        pytest.skip("a prompt past the window takes minutes on the host emulation; the windowed kernels run there in tests/test_kv8_engine.py")
    n = 70
    cfg, w, m1, cos, sin = _mk(oracle, dev, Q4KM(oracle), F8, sliding_window=40)
    _, _, m2, _, _ = _mk(oracle, dev, Q4KM(oracle), F8, sliding_window=40)
    for m in (m1, m2):
        m.set_kv_scales(0.037, 0.11)
    prompt = [(1000 + 37 * i) % cfg.vocab_size for i in range(n)]
    m1.prefill(prompt[:33], 0)
    lp = m1.prefill(prompt[33:], 33)
    for pos, t in enumerate(prompt):
        m2.set_state([t], [pos])
        ld = m2.forward_logits(1)[0]
    assert torch.equal(lp, ld)
    for k1, k2, v1, v2 in zip(m1.key_caches, m2.key_caches, m1.value_caches, m2.value_caches):
        assert torch.equal(k1, k2) and torch.equal(v1, v2)


def test_batched_steps_equal_single_steps_on_fp8_pages(oracle, dev, request):
    """batches of 2 (vector-ALU image route), 4 and 8 (matrix-core route): every sequence gets the logits and the page bytes it gets alone"""
    import torch
    emu = request.config.getoption("--host-emulation")
    npos, sizes = (1, (4, 2)) if emu else (3, (8, 4, 2))
    nseq = max(sizes)
    cfg, w, m, cos, sin = _mk(oracle, dev, Q4KM(oracle), F8, max_batch=8)
    _, _, m1, _, _ = _mk(oracle, dev, Q4KM(oracle), F8, max_batch=8)
    for mm in (m, m1):
        mm.set_kv_scales(0.037, 0.11)
    toks = [[(17 * s + 5 * p + 3) % cfg.vocab_size for p in range(npos)] for s in range(nseq)]
    alone, pages = [], []
    for s in range(nseq):  # m1's sequence 0 plays sequence s from position 0 (its pages are overwritten)
        alone.append([])
        for p in range(npos):
            m1.set_state([toks[s][p]], [p])
            alone[s].append(m1.forward_logits(1)[0].clone())
        pages.append([c[int(m1.block_tables[0, 0])].clone() for c in m1.key_caches + m1.value_caches])
    for b in sizes:
        for pos in range(npos):
            m.set_state([toks[s][pos] for s in range(b)], [pos] * b)
            both = m.forward_logits(b)
            for s in range(b):
                assert torch.equal(both[s], alone[s][pos]), f"b = {b}: sequence {s} at position {pos} differs from its single-sequence step"
        for s in range(b):
            mine = [c[int(m.block_tables[s, 0])] for c in m.key_caches + m.value_caches]
            assert all(torch.equal(x, y) for x, y in zip(mine, pages[s])), f"b = {b}: page bytes of sequence {s} differ"


def test_captured_chained_graph_equals_eager_and_new_scales_drop_it(oracle, dev, request):
    import torch
    if request.config.getoption("--host-emulation"):
        pytest.skip("graph capture needs the device")
    cfg, w, m, cos, sin = _mk(oracle, dev, Q4KM(oracle), F8)
    _, _, m2, _, _ = _mk(oracle, dev, Q4KM(oracle), F8)
    for mm in (m, m2):
        mm.set_kv_scales(0.037, 0.11)
    prompt = [(1000 + i) % cfg.vocab_size for i in range(20)]
    lt = m.prefill(prompt, 0)
    assert torch.equal(m2.prefill(prompt, 0), lt)
    eager, tok = [], int(lt.argmax())
    first = tok
    for i in range(16):
        m.set_state([tok], [len(prompt) + i])
        tok = int(m.forward_logits(1)[0].argmax())
        eager.append(tok)
    m2.set_state([first], [len(prompt)])
    m2.step_counter.zero_()
    m2.capture_decode_graph(1)
    assert m2._graph_chained, "the decode engine's batch-1 graph should be the chained step"
    for _ in range(16):
        m2.replay()
    torch.cuda.synchronize()
    assert m2.tokens_out[0, :16].tolist() == eager
    assert torch.equal(m2.logits[0], m.logits[0])
    for k1, k2 in zip(m.key_caches + m.value_caches, m2.key_caches + m2.value_caches):
        assert torch.equal(k1, k2)
    m2.set_kv_scales(0.05, 0.11)  # launch arguments of the captured kernels: the graph of the old scales must not run again
    with pytest.raises(RuntimeError, match="no decode graph"):
        m2.replay()


def test_kv_cache_bytes_and_refusals(oracle, dev, request):
    from mistralrs_amd.llama import Llama, LlamaConfig
    cfg, w, m, cos, sin = _mk(oracle, dev, Q4KM(oracle), F8)
    _, _, mb, _, _ = _mk(oracle, dev, Q4KM(oracle), "bf16")
    assert 2 * m.kv_cache_bytes == mb.kv_cache_bytes and m.kv_cache_bytes == 2 * cfg.num_layers * m.num_blocks * cfg.num_kv_heads * cfg.head_dim * cfg.block_size
    prompt = [(1000 + i) % cfg.vocab_size for i in range(5)]
    # the bf16 prompt modes read and write bf16 pages
    for mode in (0, 2):
        m.set_prefill_mode(mode)
        with pytest.raises(ValueError, match="bf16"):
            m.prefill(prompt, 0)
        assert not m.prefill_is_exact and int(m.key_caches[0].count_nonzero()) == 0  # nothing ran: the pages are untouched
    m.set_prefill_mode(1)
    assert m.prefill_is_exact
    # non-engine decode modes
    with pytest.raises(ValueError, match="decode-engine feature"):
        Llama(LlamaConfig(hidden_size=512, intermediate_size=1024, num_layers=1, num_heads=4, num_kv_heads=2, vocab_size=64, head_dim=128, max_position_embeddings=256,
                          max_context_len=64, decode_engine=False, kv_dtype=F8), dev)
    m._chk(m._L.mrs_llama_set_mode(m._h, 1))
    m.set_state([1], [0])
    assert m._L.mrs_llama_forward_logits(m._h, 1, m._stream()) != 0 and "FP8 KV pages need the decode engine" in m._err()
    m._chk(m._L.mrs_llama_set_mode(m._h, 2))
    # scales: finite and > 0, a scalar or one per layer; only on an FP8 model
    for bad in ((0.0, 1.0), (1.0, -2.0), (float("nan"), 1.0), (1.0, float("inf")), ([1.0, 1.0, 1.0], 1.0)):
        with pytest.raises(ValueError, match="set_kv_scales"):
            m.set_kv_scales(*bad)
    assert m._L.mrs_llama_set_kv_scales(m._h, 0, C.c_float(-1.0), C.c_float(1.0)) != 0 and "finite and > 0" in m._err()
    assert m._L.mrs_llama_set_kv_scales(m._h, cfg.num_layers, C.c_float(1.0), C.c_float(1.0)) != 0
    with pytest.raises(ValueError, match="no FP8 KV pages"):
        mb.set_kv_scales(1.0, 1.0)
    with pytest.raises(ValueError, match="kv_dtype must be"):
        Llama(LlamaConfig(hidden_size=512, intermediate_size=1024, num_layers=1, num_heads=4, num_kv_heads=2, vocab_size=64, head_dim=128, max_position_embeddings=256,
                          max_context_len=64, kv_dtype="f8e5m2"), dev)
    m.set_kv_scales([0.5, 0.25], 2.0)  # and good ones pass


def test_paged_engine_with_a_preemption_equals_plain_greedy_decoding_on_fp8_pages(oracle, dev, request):
    """Two greedy sequences through PagedEngine on a pool that holds both prompts but not both continuations: one is preempted and recomputed; the tokens equal
    Llama-level greedy decoding of the same prompts (PagedEngine needed no change for FP8 pages)."""
    from mistralrs_amd.kv_cache_manager import KVCacheManager
    from mistralrs_amd.scheduler import PagedAttentionScheduler, PagedEngine, SchedulerConfig, Sequence
    if request.config.getoption("--host-emulation"):
        pytest.skip("minutes on the host emulation; the bookkeeping runs on the fake runner in the CPU suite")
    lens = [(30, 8), (31, 8)]  # both cross into a second 32-token block while they decode
    cfg, w, m, cos, sin = _mk(oracle, dev, Q4KM(oracle), F8, max_batch=8, max_ctx=128, max_new=8)
    m.set_kv_scales(0.037, 0.11)
    prompts = [[(1000 + 13 * i + 7 * j * j) % cfg.vocab_size for j in range(n)] for i, (n, _) in enumerate(lens)]
    mgr = KVCacheManager(POOL, cfg.block_size, True, [0])
    sched = PagedAttentionScheduler(SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=16, max_decode_steps_before_prefill=3), mgr)
    seqs = [Sequence(id=i + 1, tokens=list(p), max_new_tokens=nn) for i, (p, (_, nn)) in enumerate(zip(prompts, lens))]
    for s in seqs:
        sched.add_seq(s)
    eng = PagedEngine(m, sched)
    eng.run(max_steps=2000)
    assert all(s.state == "done" and len(s.generated) == nn for s, (_, nn) in zip(seqs, lens))
    assert eng.steps["preemptions"] > 0, eng.steps
    assert mgr.num_free_blocks() == mgr.num_usable_blocks()
    for s, p, (_, nn) in zip(seqs, prompts, lens):
        _, _, solo, _, _ = _mk(oracle, dev, Q4KM(oracle), F8, max_batch=8, max_ctx=128, max_new=8)
        solo.set_kv_scales(0.037, 0.11)
        toks = list(p)
        for pos in range(len(p) + nn - 1):
            solo.set_state([toks[pos]], [pos])
            lg = solo.forward_logits(1)[0]
            if pos >= len(p) - 1:
                toks.append(int(lg.argmax()))
        assert toks[len(p):] == s.generated, (s.id, toks[len(p):], s.generated)


POOL = 3  # 32-token blocks: both prompts fit (one block each), both continuations (two each) do not
